"""Routing of registered-key Ed25519 lanes to the keyed verifier on the GPU (K14:
cordahip_vkey_set_routing, cordahip_vkey_route_stats) through every call that reaches
ed_verify_enqueue: the dense device call, both device signed-tx calls, the host generic
batch and the host signed-tx batch. Every status is compared with the C oracle (or the golden
vectors), not only with the unrouted call; cordahip_vkey_route_stats shows which engine ran.
Outputs are prefilled with 0xA5 and sit between guard bytes. Every test that turns routing on
uses a context of its own, so the session engine never changes path."""
import collections
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from corda_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, UNSUPPORTED, EMPTY = _lib.OK, 1, 2, 3, 4, _lib.EMPTY
UNKNOWN = _lib.VERIFY_UNKNOWN_KEY
ED, K1, R1, SPHINCS = 4, 2, 3, 5
PAD = 100
TPAD = 128  # the signed-tx calls' outputs keep their 16-byte alignment
A5_WORD = 0xA5A5A5A5A5A5A5A5


def csign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


def oracle_dense(oracle, pubs, sigs, msgs, msg_len):
    """oracle_ed25519_verify_batch over dense rows (doVerify rules)."""
    n = len(pubs)
    k = np.frombuffer(b"".join(pubs), np.uint8).copy()
    s = np.frombuffer(b"".join(sigs), np.uint8).copy()
    m = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()
    want = np.zeros(n, np.uint8)
    oracle.oracle_ed25519_verify_batch(n, k.ctypes.data, s.ctypes.data, m.ctypes.data, msg_len, want.ctypes.data, 8)
    return want


def verdict_bits(words, n):
    return np.array([(int(words[i >> 6]) >> (i & 63)) & 1 for i in range(n)], np.uint8)


def dense_call(eng, pubs, sigs, msgs, msg_len, with_verdict=True):
    """cordahip_ed25519_verify_device over the lanes, outputs 0xA5 between guards. Returns the
    statuses; checks the guards, and (with_verdict) bit = status OK and zero bits past n."""
    import torch
    dev = torch.device("cuda:0")
    n = len(pubs)
    words = (n + 63) // 64
    t_key = torch.from_numpy(np.frombuffer(b"".join(pubs), np.uint8).reshape(n, 32).copy()).to(dev)
    t_sig = torch.from_numpy(np.frombuffer(b"".join(sigs), np.uint8).reshape(n, 64).copy()).to(dev)
    t_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).reshape(n, msg_len).copy()).to(dev) \
        if msg_len else torch.empty((n, 0), dtype=torch.uint8, device=dev)
    t_st = torch.full((PAD + n + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    t_vd = torch.full((2 + words + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    eng.ed25519_verify_device(t_key, t_sig, t_msg, t_st[PAD:PAD + n], t_vd[2:2 + words] if with_verdict else None,
                              stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    st_all, vd_all = t_st.cpu().numpy(), t_vd.cpu().numpy().view(np.uint64)
    assert (st_all[:PAD] == 0xA5).all() and (st_all[PAD + n:] == 0xA5).all()
    assert (vd_all[:2] == A5_WORD).all() and (vd_all[2 + words:] == A5_WORD).all()
    got = st_all[PAD:PAD + n].copy()
    if with_verdict:
        bits = verdict_bits(vd_all[2:2 + words], words * 64)
        assert np.array_equal(bits[:n], (got == OK).astype(np.uint8)) and not bits[n:].any()
    else:
        assert (vd_all == A5_WORD).all()
    return got


def canonical(pub):
    """EdDSAPublicKey.Abyte of the key bytes (None: they do not decode)."""
    import i2p_ed25519 as ref
    p = ref.decode_i2p(pub)
    return None if p is None else ref.encode(p)


# ---- 1. golden vectors -------------------------------------------------------------------
def test_golden_vectors_routed(ed_vectors, oracle):
    """Every golden lane, none left out. The 476 lanes a dense call can carry (32-byte key,
    64-byte signature) run through cordahip_ed25519_verify_device per message length, routing
    off and then on, in every round of registered keys; the 7 others (signature or key of another
    length, decided before the engine) run through cordahip_sig_verify with routing on."""
    from corda_amd.engine import Engine
    assert len(ed_vectors) == 483
    dense = [v for v in ed_vectors if len(v["pub"]) == 32 and len(v["sig"]) == 64]
    other = [v for v in ed_vectors if not (len(v["pub"]) == 32 and len(v["sig"]) == 64)]
    assert len(dense) == 476 and len(other) == 7
    by_len = collections.defaultdict(list)
    for v in dense:
        by_len[len(v["msg"])].append(v)
    assert len(by_len) >= 10 and 0 in by_len
    cats = collections.Counter(v["cat"] for v in dense)
    assert cats["key_noncanonical_y"] == 38 and cats["key_identity_signbit"] == 8 and cats["key_mixed_order"] == 34
    keys = [k for k in dict.fromkeys(v["pub"] for v in ed_vectors if len(v["pub"]) == 32) if canonical(k) is not None]
    assert len(keys) == 241
    keyed_cats = collections.Counter()
    keyed_per_round = []
    with Engine(1) as eng:
        for g in range(0, len(keys), _lib.VKEY_MAX_KEYS):
            group = keys[g:g + _lib.VKEY_MAX_KEYS]
            ids = []
            for k in group:
                kid, st = eng.vkey_add_ed25519(k)
                assert st == OK
                ids.append(kid)
            stored = {canonical(k) for k in group}  # what the records hold
            want_keyed = 0
            for ml, lanes in sorted(by_len.items()):
                args = ([v["pub"] for v in lanes], [v["sig"] for v in lanes], [v["msg"] for v in lanes], ml)
                golden = np.array([v["status"] for v in lanes], np.uint8)
                eng.vkey_set_routing(False)
                before = eng.vkey_route_stats()
                off = dense_call(eng, *args)
                assert eng.vkey_route_stats() == before  # routing off: counted nowhere
                eng.vkey_set_routing(True)
                on = dense_call(eng, *args)
                for name, got in (("off", off), ("on", on)):
                    wrong = [(name, v["cat"], v["note"], int(s), v["status"]) for v, s in zip(lanes, got)
                             if s != v["status"]]
                    assert not wrong, wrong[:10]
                assert np.array_equal(on, golden)
                keyed = [v for v in lanes if v["pub"] in stored]
                after = eng.vkey_route_stats()
                assert (after[0] - before[0], after[1] - before[1]) == (len(keyed), len(lanes) - len(keyed)), (g, ml)
                want_keyed += len(keyed)
                for v in keyed:
                    keyed_cats[v["cat"]] += 1
            # the lanes a dense call cannot carry: the host batch, routed
            st, _ = eng.verify_batch([ED] * len(other), [v["pub"] for v in other], [v["sig"] for v in other],
                                     [v["msg"] for v in other])
            assert [int(s) for s in st] == [v["status"] for v in other]
            keyed_per_round.append(want_keyed)
            eng.vkey_set_routing(False)
            for kid in ids:
                eng.vkey_remove(kid)
    assert len(keyed_per_round) == 4 and max(keyed_per_round) > 0 and sum(keyed_per_round) > 100, keyed_per_round
    # a lane with a non-canonical encoding matches only through a canonical twin among the keys
    assert keyed_cats["valid"] > 0, keyed_cats
    non_canonical = [v for v in dense if canonical(v["pub"]) not in (None, v["pub"])]
    assert non_canonical and {"key_noncanonical_y", "key_identity_signbit"} <= {v["cat"] for v in non_canonical}


# ---- 2. partition edges --------------------------------------------------------------------
EDGE_SIZES = (1, 63, 64, 65, 5 * 64 + 37)


def edge_patterns(n):
    """name -> is-K per lane; a keyed count of exactly 255 / 256 / 257 needs n above it."""
    pats = {"all_k": [True] * n, "all_u": [False] * n, "alternating": [i % 2 == 0 for i in range(n)],
            "k_last": [i == n - 1 for i in range(n)]}
    for c in (255, 256, 257):
        if n > c:  # the U lanes spread over the batch, K everywhere else
            u = set(int(x) for x in np.linspace(0, n - 1, n - c).round())
            assert len(u) == n - c
            pats["keyed_%d" % c] = [i not in u for i in range(n)]
    return pats


def partition_edges(eng, oracle):
    """One registered key K, one unregistered U, fresh signatures with 1 in 7 corrupted (an S bit
    flipped) on both; every pattern x size x verdict NULL / non-NULL x msg_len 32 / 0. Returns the
    number of dense calls made."""
    nmax = max(EDGE_SIZES)
    seed_k, seed_u = hashlib.sha256(b"route-K").digest(), hashlib.sha256(b"route-U").digest()
    pool = {True: [], False: []}
    msgs = [hashlib.sha256(b"route-edge-%d" % i).digest() for i in range(nmax)]
    for is_k, seed in ((True, seed_k), (False, seed_u)):
        for i in range(nmax):
            pub, sig = csign(oracle, seed, msgs[i])
            if i % 7 == 3:
                sig = sig[:32 + i % 31] + bytes([sig[32 + i % 31] ^ (1 << (i % 8))]) + sig[33 + i % 31:]
            pool[is_k].append((pub, sig))
    kid, st = eng.vkey_add_ed25519(pool[True][0][0])
    assert st == OK
    eng.vkey_set_routing(True)
    calls = 0
    seen = set()
    for n in EDGE_SIZES:
        for name, is_k in edge_patterns(n).items():
            pubs = [pool[k][i][0] for i, k in enumerate(is_k)]
            sigs = [pool[k][i][1] for i, k in enumerate(is_k)]
            for ml in (32, 0):
                m = [x[:ml] for x in msgs[:n]]
                want = oracle_dense(oracle, pubs, sigs, m, ml)
                if ml == 0:
                    assert (want == EMPTY).all()
                elif n > 64:
                    assert (want == OK).any() and (want == BAD_SIG).any()
                for with_verdict in (True, False):
                    before = eng.vkey_route_stats()
                    got = dense_call(eng, pubs, sigs, m, ml, with_verdict)
                    bad = np.nonzero(got != want)[0]
                    assert not len(bad), (n, name, ml, with_verdict, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])
                    after = eng.vkey_route_stats()
                    assert (after[0] - before[0], after[1] - before[1]) == (sum(is_k), n - sum(is_k)), (n, name, ml)
                    calls += 1
            seen.add(name)
    assert seen == {"all_k", "all_u", "alternating", "k_last", "keyed_255", "keyed_256", "keyed_257"}
    eng.vkey_set_routing(False)
    eng.vkey_remove(kid)
    return calls


def test_partition_edges(oracle):
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        assert partition_edges(eng, oracle) == (4 * 5 + 3) * 4


def run_self(func, env):
    """`func` of this module in a fresh process (the variables in env are read once per process)."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_vkey_route as t; t.%s()"
            % (ROOT, os.path.join(ROOT, "tests"), func))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def main_partition_edges():
    from conftest import load_oracle
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        print(json.dumps({"calls": partition_edges(eng, load_oracle())}))


def test_partition_edges_small_workspace_subprocess():
    """A workspace of 128 lanes: the generic list of the larger batches spans several chunks, and
    launches fall wholly past the count (every lane keyed: all of them)."""
    assert run_self("main_partition_edges", {"CORDAHIP_ED25519_WS_LANES": "128"})["calls"] == (4 * 5 + 3) * 4


# ---- 3 / 5. signed transactions ---------------------------------------------------------------
NTX = 300
NO_SIG_TX = 123


def tx_corpus(eng, oracle):
    """300 cash-issue-shaped transactions of two signatures each -- the notary K, then a fresh
    key -- over their ids; signatures of each kind corrupted at chosen positions; one transaction
    without signatures. The expected statuses come from the oracle over (key, signature, id)."""
    from corda_amd.corpus import cash_issue_items
    rng = np.random.default_rng(1514)
    blob, items, _ = cash_issue_items(rng.integers(0, 256, (NTX, 32), dtype=np.uint8),
                                      rng.integers(0, 256, (NTX, 32), dtype=np.uint8), bytes(range(32)),
                                      rng.integers(1, 10**9, NTX), rng.integers(-2**63, 2**63 - 1, NTX))
    it = items.reshape(-1).copy()
    host_it = it.copy()
    host_it["data"] += np.uint64(blob.ctypes.data)
    hb, ho = _lib.kryo_encode_array(host_it)
    leaves = [[hb[int(ho[5 * t + j]):int(ho[5 * t + j + 1])].tobytes() for j in range(5)] for t in range(NTX)]
    ids, _ = eng.tx_ids(leaves)
    out = ctypes.create_string_buffer(32)
    for t in (0, NO_SIG_TX, NTX - 1):  # the ids themselves against the oracle
        flat = np.frombuffer(b"".join(leaves[t]), np.uint8).copy()
        off = np.zeros(6, np.uint64)
        off[1:] = np.cumsum([len(x) for x in leaves[t]])
        assert oracle.oracle_tx_id(flat.ctypes.data, off.ctypes.data, 5, out) == 0 and out.raw == ids[t].tobytes()
    seed_k = hashlib.sha256(b"route-notary").digest()
    pub_k = csign(oracle, seed_k, b"x")[0]
    per_tx, keys, sigs, msgs = [], [], [], []
    for t in range(NTX):
        per = []
        if t != NO_SIG_TX:
            m = ids[t].tobytes()
            for q, seed in enumerate((seed_k, hashlib.sha256(b"route-fresh-%d" % t).digest())):
                pub, sg = csign(oracle, seed, m)
                if (q == 0 and t % 13 == 4) or (q == 1 and t % 17 == 6) or t == 200:  # t = 200: both
                    sg = sg[:40] + bytes([sg[40] ^ 4]) + sg[41:]
                per.append((ED, pub, sg))
                keys.append(pub)
                sigs.append(sg)
                msgs.append(m)
        per_tx.append(per)
    want_sig = oracle_dense(oracle, keys, sigs, msgs, 32)
    tso = np.zeros(NTX + 1, np.int64)
    tso[1:] = np.cumsum([len(p) for p in per_tx])
    want_fb, want_tx = [], []
    for t in range(NTX):
        st = want_sig[tso[t]:tso[t + 1]]
        bad = np.nonzero(st != OK)[0]
        want_fb.append(int(bad[0]) if len(bad) else -1)
        want_tx.append(_lib.TX_NO_SIGNATURES if not len(st) else int(st[bad[0]]) if len(bad) else 0)
    n_k = sum(k == pub_k for k in keys)
    assert n_k == NTX - 1 and len(keys) == 2 * (NTX - 1)
    assert (want_sig == BAD_SIG).sum() == len([t for t in range(NTX) if t % 13 == 4 and t not in (NO_SIG_TX, 200)]) + \
        len([t for t in range(NTX) if t % 17 == 6 and t not in (NO_SIG_TX, 200)]) + 2
    assert want_fb[200] == 0 and 1 in want_fb
    return dict(blob=blob, it=it, leaves=leaves, ids=ids, pub_k=pub_k, per_tx=per_tx, keys=keys, sigs=sigs, tso=tso,
                want_sig=want_sig, want_fb=np.array(want_fb), want_tx=np.array(want_tx, np.uint8), n_k=n_k)


def device_tx_calls(eng, c):
    """Both device signed-tx calls over the corpus: name -> (txid, tx_status, first_bad, sig_status)."""
    import torch
    dev = torch.device("cuda:0")
    nsig = len(c["keys"])
    K = torch.tensor(np.frombuffer(b"".join(c["keys"]), np.uint8).reshape(-1, 32), device=dev)
    S = torch.tensor(np.frombuffer(b"".join(c["sigs"]), np.uint8).reshape(-1, 64), device=dev)
    d_so = torch.from_numpy(c["tso"]).to(dev)
    d_tlo = torch.from_numpy(np.arange(0, 5 * NTX + 1, 5, dtype=np.int64)).to(dev)
    out = {}
    for name in ("leaf", "comp"):
        txid = torch.full((TPAD + NTX + TPAD, 32), 0xA5, dtype=torch.uint8, device=dev)
        st = torch.full((TPAD + NTX + TPAD,), 0xA5, dtype=torch.uint8, device=dev)
        fb = torch.full((2 + NTX + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
        sst = torch.full((TPAD + nsig + TPAD,), 0xA5, dtype=torch.uint8, device=dev)
        o = (txid[TPAD:TPAD + NTX], st[TPAD:TPAD + NTX], fb[2:2 + NTX], sst[TPAD:TPAD + nsig])
        if name == "leaf":
            flat = [x for tx in c["leaves"] for x in tx]
            lb = torch.tensor(np.frombuffer(b"".join(flat), np.uint8), device=dev)
            lo = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64), device=dev)
            eng.signed_tx_verify_ed25519_device(lb, lo, d_tlo, d_so, K, S, *o)
        else:
            d_items = torch.from_numpy(np.ascontiguousarray(c["it"]).view(np.uint8).copy()).to(dev)
            d_blob = torch.from_numpy(np.ascontiguousarray(c["blob"])).to(dev)
            eng.signed_txcomp_verify_ed25519_device(d_items, len(c["it"]), d_blob, d_tlo, d_so, K, S, *o, group=5)
        torch.cuda.synchronize()
        for buf, lo_, hi_ in ((txid, TPAD, TPAD + NTX), (st, TPAD, TPAD + NTX), (sst, TPAD, TPAD + nsig)):
            b = buf.cpu().numpy()
            assert (b[:lo_] == 0xA5).all() and (b[hi_:] == 0xA5).all(), name
        b = fb.cpu().numpy().view(np.uint64)
        assert (b[:2] == A5_WORD).all() and (b[2 + NTX:] == A5_WORD).all(), name
        out[name] = tuple(x.cpu().numpy().copy() for x in o)
    return out


def main_device_tx():
    from conftest import load_oracle
    from corda_amd.engine import Engine
    oracle = load_oracle()
    res = {}
    with Engine(1) as eng:
        c = tx_corpus(eng, oracle)
        kid, st = eng.vkey_add_ed25519(c["pub_k"])
        assert st == OK
        runs = {}
        for mode in ("off", "on"):
            eng.vkey_set_routing(mode == "on")
            before = eng.vkey_route_stats()
            runs[mode] = device_tx_calls(eng, c)
            after = eng.vkey_route_stats()
            res["stats_" + mode] = [after[0] - before[0], after[1] - before[1]]
            for name, (txid, tst, fb, sst) in runs[mode].items():
                skip = np.arange(NTX) != NO_SIG_TX  # a transaction without signatures: its id is not asked for
                assert np.array_equal(txid[skip], c["ids"][skip]), (mode, name)
                assert np.array_equal(sst, c["want_sig"]), (mode, name, np.nonzero(sst != c["want_sig"])[0][:8])
                assert np.array_equal(fb, c["want_fb"]), (mode, name)
                assert np.array_equal(tst, c["want_tx"]), (mode, name)
        for name in ("leaf", "comp"):
            assert all(np.array_equal(a, b) for a, b in zip(runs["off"][name], runs["on"][name])), name
        res["n_k"], res["nsig"] = c["n_k"], len(c["keys"])
        eng.vkey_set_routing(False)
        eng.vkey_remove(kid)
    print(json.dumps(res))


def test_device_signed_tx_both_calls_subprocess():
    """Chunks of 128 signatures: the remainder and four full chunks alternate between the two
    workspace slots and streams, each routed on its own."""
    res = run_self("main_device_tx", {"CORDAHIP_DEVICE_ED_CHUNK": "128"})
    assert res["nsig"] == 598 and res["n_k"] == 299
    assert res["stats_off"] == [0, 0]
    assert res["stats_on"] == [2 * 299, 2 * 299]  # two calls; every notary lane keyed, none lost


@pytest.mark.parametrize("slices", ["default", "1", "3", "16"])
def test_host_signed_tx_two_tickets(oracle, slices, monkeypatch):
    from corda_amd.engine import Engine
    if slices == "default":
        monkeypatch.delenv("CORDAHIP_TX_SLICES", raising=False)
    else:
        monkeypatch.setenv("CORDAHIP_TX_SLICES", slices)
    monkeypatch.setenv("CORDAHIP_TX_SIG_CHUNK", "100")  # several pipeline chunks per call
    with Engine(1) as eng:
        c = tx_corpus(eng, oracle)
        kid, st = eng.vkey_add_ed25519(c["pub_k"])
        assert st == OK
        eng.vkey_set_routing(True)
        before = eng.vkey_route_stats()
        tickets = [eng.signed_tx_verify(c["leaves"], c["per_tx"], async_=True) for _ in range(2)]
        for t in reversed(tickets):
            ids, tst, fb, sst = t.wait()
            skip = np.arange(NTX) != NO_SIG_TX
            assert np.array_equal(ids[skip], c["ids"][skip])
            assert np.array_equal(sst, c["want_sig"]), np.nonzero(sst != c["want_sig"])[0][:8]
            assert np.array_equal(fb, c["want_fb"]) and np.array_equal(tst, c["want_tx"])
        after = eng.vkey_route_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (2 * c["n_k"], 2 * (len(c["keys"]) - c["n_k"]))
        eng.vkey_set_routing(False)
        eng.vkey_remove(kid)


# ---- 4. the host generic batch ------------------------------------------------------------------
def test_host_generic_batch_two_tickets(oracle, ec_vectors):
    from corda_amd.engine import Engine
    seed_k, seed_u = hashlib.sha256(b"route-gen-K").digest(), hashlib.sha256(b"route-gen-U").digest()
    pub_k = csign(oracle, seed_k, b"x")[0]
    lanes = []  # (scheme, key, sig, msg)
    for i in range(150):  # Ed25519 lanes of two message lengths on K and U, 1 in 5 corrupted
        msg = (hashlib.sha512(b"route-gen-%d" % i).digest())[:32 if i % 3 else 50]
        pub, sig = csign(oracle, seed_k if i % 2 else seed_u, msg)
        if i % 5 == 2:
            sig = sig[:33] + bytes([sig[33] ^ 0x20]) + sig[34:]
        lanes.append((ED, pub, sig, msg))
    for scheme in (K1, R1):  # ECDSA lanes of both curves, accepted and rejected
        for cat in ("valid", "valid_compressed", "sig_bitflip"):
            lanes += [(scheme, v["pub"], v["sig"], v["msg"]) for v in ec_vectors
                      if v["scheme"] == scheme and v["cat"] == cat][:6]
    m32 = hashlib.sha256(b"route-gen-odd").digest()
    good = csign(oracle, seed_k, m32)[1]
    lanes.append((ED, pub_k, b"", m32))              # an empty signature
    lanes.append((ED, pub_k, good[:63], m32))        # a 63-byte signature
    lanes.append((SPHINCS, pub_k, good, m32))        # an unsupported scheme
    lanes.append((ED, pub_k[:31], good, m32))        # a 31-byte key
    lanes.append((ED, pub_k, good, m32))
    order = np.random.default_rng(4).permutation(len(lanes))
    lanes = [lanes[i] for i in order]

    def want(is_valid):
        out = []
        for s, k, g, m in lanes:
            if s == ED:
                f = oracle.oracle_ed25519_is_valid if is_valid else oracle.oracle_ed25519_verify
                out.append(f(k, len(k), g, len(g), m, len(m)))
            elif s in (K1, R1):
                f = oracle.oracle_ecdsa_is_valid if is_valid else oracle.oracle_ecdsa_verify
                out.append(f(s, k, len(k), g, len(g), m, len(m)))
            else:
                out.append(UNSUPPORTED)
        return np.array(out, np.uint8)

    w0, w1 = want(False), want(True)
    assert {OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, UNSUPPORTED, EMPTY} <= set(w0.tolist())
    assert EMPTY not in set(w1.tolist()) and (w0 != w1).any()
    on_k = sum(s == ED and k == pub_k for s, k, _, _ in lanes)
    ed32 = sum(s == ED and len(k) == 32 for s, k, _, _ in lanes)
    assert on_k == 75 + 3
    args = ([x[0] for x in lanes], [x[1] for x in lanes], [x[2] for x in lanes], [x[3] for x in lanes])
    with Engine(1) as eng:
        off0, _ = eng.verify_batch(*args)
        assert np.array_equal(off0, w0)
        kid, st = eng.vkey_add_ed25519(pub_k)
        assert st == OK
        eng.vkey_set_routing(True)
        before = eng.vkey_route_stats()
        t0 = eng.verify_batch(*args, async_=True)
        t1 = eng.verify_batch(*args, async_=True, is_valid=True)
        for t, w in ((t1, w1), (t0, w0)):
            st, vd = t.wait()
            bad = np.nonzero(st != w)[0]
            assert not len(bad), [(int(i), lanes[i][0], int(st[i]), int(w[i])) for i in bad[:8]]
            assert np.array_equal(verdict_bits(vd, len(lanes)), (w == OK).astype(np.uint8))
        after = eng.vkey_route_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (2 * on_k, 2 * (ed32 - on_k))
        st, _ = eng.verify_batch(*args)  # the synchronous call
        assert np.array_equal(st, w0)
        eng.vkey_set_routing(False)
        eng.vkey_remove(kid)


# ---- 6. registry changes ---------------------------------------------------------------------
def test_registry_changes_under_routing(oracle):
    from corda_amd.engine import Engine
    n = 200
    seed_k, seed_u = hashlib.sha256(b"route-reg-K").digest(), hashlib.sha256(b"route-reg-U").digest()
    msgs = [hashlib.sha256(b"route-reg-%d" % i).digest() for i in range(n)]
    pubs, sigs = [], []
    for i in range(n):
        pub, sig = csign(oracle, seed_k if i % 3 else seed_u, msgs[i])
        if i % 7 == 1:
            sig = sig[:50] + bytes([sig[50] ^ 1]) + sig[51:]
        pubs.append(pub)
        sigs.append(sig)
    pub_k = csign(oracle, seed_k, b"x")[0]
    n_k = sum(p == pub_k for p in pubs)
    want = oracle_dense(oracle, pubs, sigs, msgs, 32)
    assert (want == OK).any() and (want == BAD_SIG).any() and 0 < n_k < n

    def run(eng):
        before = eng.vkey_route_stats()
        got = dense_call(eng, pubs, sigs, msgs, 32)
        after = eng.vkey_route_stats()
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        assert UNKNOWN not in got
        return after[0] - before[0], after[1] - before[1]

    with Engine(1) as eng:
        assert eng.vkey_route_stats() == (0, 0)
        eng.vkey_set_routing(True)
        assert run(eng) == (0, 0)  # no key registered: today's path, nothing counted
        ec = bytes.fromhex("0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798")  # secp256k1's G
        ec_id, st = eng.vkey_add_ecdsa(K1, ec)  # an ECDSA key alone is no reason to route
        assert st == OK
        assert run(eng) == (0, 0)
        def mem():
            u = ctypes.c_uint64()
            assert _lib.lib().cordahip_device_mem(eng.ctx, 0, ctypes.byref(u), None, None) == 0
            return u.value

        unrouted = mem()  # the workspace of n lanes is there already
        a, st = eng.vkey_add_ed25519(pub_k)
        assert st == OK
        assert run(eng) == (n_k, n - n_k)
        # what routing adds to the device's account: the key tables (ed25519_vkey.hpp), the two
        # cumulative counters, and slot 0's scratch of 12 B per lane behind a 64-byte header,
        # allocated for at least 2^16 lanes (ed25519_route.hpp kRouteMinLanes)
        vkey_bytes = 65 * 512 * 1024 + 64 * 64 + 64
        scratch = 64 + 12 * (1 << 16)
        assert n < 1 << 16 and mem() - unrouted == vkey_bytes + 16 + scratch
        # the scratch leaves the account with the workspace; the counters stay, routing works again
        held, tot = mem(), eng.vkey_route_stats()
        assert _lib.lib().cordahip_trim(eng.ctx) == 0
        assert held - mem() > scratch and eng.vkey_route_stats() == tot
        assert run(eng) == (n_k, n - n_k)
        eng.vkey_remove(a)
        assert run(eng) == (0, 0)  # K removed: the same statuses from the generic engine, nothing counted
        other, st = eng.vkey_add_ed25519(csign(oracle, seed_u[::-1], b"x")[0])  # takes K's old slot
        assert st == OK and (other & 63) == (a & 63)
        assert run(eng) == (0, n)  # a live key that no lane carries: all generic, counted
        b, st = eng.vkey_add_ed25519(pub_k)  # the same bytes again: a new id, live
        assert st == OK and b != a
        assert run(eng) == (n_k, n - n_k)
        c, st = eng.vkey_add_ed25519(pub_k)  # the same bytes in two slots: either serves
        assert st == OK
        assert run(eng) == (n_k, n - n_k)
        eng.vkey_remove(b)
        assert run(eng) == (n_k, n - n_k)
        eng.vkey_set_routing(False)
        assert run(eng) == (0, 0)
        assert ctypes.c_int(_lib.lib().cordahip_vkey_route_stats(eng.ctx, 7, None, None)).value == _lib.ERR_INVALID_ARG


# ---- 7. the stream call -------------------------------------------------------------------------
def test_stream_call_is_routed(oracle):
    """cordahip_stream_verify reaches ed_verify_enqueue chunk by chunk, so its Ed25519 section is
    routed too (the ECDSA section is empty here): statuses against the oracle, the split in the stats."""
    from corda_amd.engine import Engine
    n = 333
    seed_k, seed_u = hashlib.sha256(b"route-stream-K").digest(), hashlib.sha256(b"route-stream-U").digest()
    msgs = [hashlib.sha256(b"route-stream-%d" % i).digest() for i in range(n)]
    pubs, sigs = [], []
    for i in range(n):
        pub, sig = csign(oracle, seed_k if i % 4 else seed_u, msgs[i])
        if i % 6 == 5:
            sig = sig[:45] + bytes([sig[45] ^ 8]) + sig[46:]
        pubs.append(pub)
        sigs.append(sig)
    pub_k = csign(oracle, seed_k, b"x")[0]
    n_k = sum(p == pub_k for p in pubs)
    want = oracle_dense(oracle, pubs, sigs, msgs, 32)
    assert (want == OK).any() and (want == BAD_SIG).any()
    ek = np.frombuffer(b"".join(pubs), np.uint8).reshape(n, 32).copy()
    es = np.frombuffer(b"".join(sigs), np.uint8).reshape(n, 64).copy()
    em = np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32).copy()
    empty = np.zeros(0, np.uint8)
    ec = (empty, np.zeros((0, 65), np.uint8), empty, np.zeros((0, 72), np.uint8), empty, np.zeros((0, 32), np.uint8),
          empty)
    with Engine(1) as eng:
        kid, st = eng.vkey_add_ed25519(pub_k)
        assert st == OK
        for on, split in ((False, (0, 0)), (True, (n_k, n - n_k))):
            eng.vkey_set_routing(on)
            before = eng.vkey_route_stats()
            got = np.full(n, 0xA5, np.uint8)
            eng.stream_verify((ek, es, em, got), ec)
            after = eng.vkey_route_stats()
            assert np.array_equal(got, want), (on, np.nonzero(got != want)[0][:8])
            assert (after[0] - before[0], after[1] - before[1]) == split, on
        eng.vkey_set_routing(False)
        eng.vkey_remove(kid)


# ---- 8. the lock order ---------------------------------------------------------------------------
def test_trim_keyed_and_routed_calls_together(oracle):
    """cordahip_trim (every buffer lock, vkey_stage.mu last), cordahip_verify_keyed (vkey_stage.mu
    around vkey_mu) and a routed dense device call (ed_mu around vkey_mu) from three threads: one
    lock order, so all three finish, with the right statuses throughout."""
    import threading
    from corda_amd.engine import Engine
    n = 130
    seed_k = hashlib.sha256(b"route-locks-K").digest()
    msgs = [hashlib.sha256(b"route-locks-%d" % i).digest() for i in range(n)]
    pairs = [csign(oracle, seed_k if i % 2 else hashlib.sha256(b"route-locks-U%d" % i).digest(), msgs[i])
             for i in range(n)]
    pubs = [p for p, _ in pairs]
    sigs = [s if i % 9 else s[:35] + bytes([s[35] ^ 2]) + s[36:] for i, (_, s) in enumerate(pairs)]
    want = oracle_dense(oracle, pubs, sigs, msgs, 32)
    pub_k = csign(oracle, seed_k, b"x")[0]
    k_lanes = [i for i in range(n) if pubs[i] == pub_k]
    errors = []
    with Engine(1) as eng:
        kid, st = eng.vkey_add_ed25519(pub_k)
        assert st == OK
        eng.vkey_set_routing(True)

        def guard(fn):
            def run():
                try:
                    for _ in range(12):
                        fn()
                except Exception as e:  # noqa: BLE001
                    errors.append(repr(e))
            return run

        def trim():
            assert _lib.lib().cordahip_trim(eng.ctx) == 0

        def keyed():
            st, _ = eng.verify_keyed_batch([kid] * len(k_lanes), [sigs[i] for i in k_lanes], [msgs[i] for i in k_lanes])
            assert np.array_equal(st, want[k_lanes])

        def routed():
            assert np.array_equal(dense_call(eng, pubs, sigs, msgs, 32), want)

        threads = [threading.Thread(target=guard(f), daemon=True) for f in (trim, keyed, routed)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert not any(t.is_alive() for t in threads), "a call did not return"
        assert not errors, errors[:3]
        keyed_lanes, generic_lanes = eng.vkey_route_stats()
        assert (keyed_lanes, generic_lanes) == (12 * len(k_lanes), 12 * (n - len(k_lanes)))
        eng.vkey_set_routing(False)
        eng.vkey_remove(kid)
