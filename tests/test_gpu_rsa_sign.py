"""RSA_SHA256 signing with registered private keys on the GPU (K19): signatures bit for bit equal
to the Python restatement (bc_rsa_pss.encode_em + sign_crt as k bytes) through the host call and
the device call, the row counts around a group, a wave and a block, the three verifiers on what
was produced, statuses and their precedence across the three signer families, registration,
chunking and tickets, a gate written on the same stream, and a context of three device replicas."""
import ctypes
import hashlib

import numpy as np
import pytest

import bc_rsa_pss as bc
import rsa_sign_model as model

pytestmark = pytest.mark.gpu

OK, EMPTY = bc.OK, bc.EMPTY
UNKNOWN, SKIPPED, FAILED, NO_ID = 14, 15, 16, 0xFFFFFFFF
RSA = 1


@pytest.fixture(scope="module")
def keys():
    return model.accepted_keys()


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own: at most 64 RSA signing keys live in one"""
    from corda_amd.engine import Engine
    with Engine(1) as e:
        yield e


@pytest.fixture(scope="module")
def reg(eng, keys):
    """every accepted golden key registered for the module: ids in key order"""
    ids = []
    for k in keys:
        kid, st, mod = eng.signer_add_rsa(*k.crt(), k.e)
        assert st == OK and kid != NO_ID and mod == k.n.to_bytes(k.k, "big"), k.name
        assert eng.signer_family(kid) == "rsa"
        ids.append(kid)
    assert len(set(ids)) == len(keys) == 11
    return ids


def device_sign(e, w, ids, msgs, salts, gate=None, device=0, msg_len=None):
    """cordahip_rsa_sign_keyed_device over rows of class w: (sigs[n, 4 w], sig_len[n], status[n])"""
    import torch
    dev = torch.device("cuda:0")
    n = len(ids)
    ln = len(msgs[0]) if msg_len is None else msg_len
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    t_ids = to(np.array(ids, np.int64).astype(np.uint32).view(np.int32))
    t_msg = to(np.frombuffer(b"".join(msgs) or bytes(1), np.uint8).reshape(n, ln) if ln else np.zeros((n, 0), np.uint8))
    t_salt = to(np.frombuffer(b"".join(salts), np.uint8).reshape(n, 32).copy())
    t_gate = None if gate is None else to(np.asarray(gate, np.uint8))
    t_sig = torch.full((n, 4 * w), 0xA5, dtype=torch.uint8, device=dev)
    t_len = torch.full((n,), -1, dtype=torch.int16, device=dev)
    t_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    e.rsa_sign_keyed_device(t_ids, t_msg, t_salt, t_sig, t_len, t_st, gate=t_gate, device=device, stream=s)
    s.synchronize()
    return t_sig.cpu().numpy(), t_len.cpu().numpy().view(np.uint16), t_st.cpu().numpy()


def row_is(sig, ln, i, want):
    """row i holds `want` at its start and zeros after it (None: a zero row of length 0)"""
    want = want or b""
    return int(ln[i]) == len(want) and sig[i][:len(want)].tobytes() == want and not sig[i][len(want):].any()


@pytest.fixture(scope="module")
def lanes(keys, reg):
    """a few lanes of every key over the message lengths, with the restatement's signatures, once"""
    out = []
    for i, k in enumerate(keys):
        for j, n in enumerate(model.MSG_LENS):
            m, s = model.message(i, n), model.salt(7 * i + j)
            out.append(dict(key=i, id=reg[i], msg=m, salt=s, want=k.sign(m, s)))
    return out


@pytest.fixture(scope="module")
def signed(eng, lanes):
    """the host call over all of them, once: (sigs, sig_len, status)"""
    return eng.rsa_sign_batch([l["id"] for l in lanes], [l["msg"] for l in lanes], [l["salt"] for l in lanes])


# ---- 1. bit-exact signatures -----------------------------------------------------------------------
def test_bit_exact_host_call(keys, lanes, signed):
    assert {k.words for k in keys} == {64, 96, 128} and {k.e for k in keys} == {3, 17, 65537, (1 << 32) - 1}
    assert {2049, 2056, 3071} <= {k.bits for k in keys}
    assert any(k.p > k.q for k in keys) and any(k.q > k.p for k in keys)
    sig, ln, st = signed
    assert sig.shape == (len(lanes), 512) and not st.any()
    for i, l in enumerate(lanes):
        assert row_is(sig, ln, i, l["want"]), (keys[l["key"]].name, len(l["msg"]))
        assert int(ln[i]) == keys[l["key"]].k


@pytest.mark.parametrize("w", (64, 96, 128))
def test_bit_exact_device_call(eng, keys, lanes, w):
    for n in model.MSG_LENS:  # dense rows: one message length a call
        rows = [l for l in lanes if keys[l["key"]].words == w and len(l["msg"]) == n]
        assert rows
        sig, ln, st = device_sign(eng, w, [l["id"] for l in rows], [l["msg"] for l in rows], [l["salt"] for l in rows])
        assert not st.any()
        for i, l in enumerate(rows):
            assert row_is(sig, ln, i, l["want"]), (keys[l["key"]].name, n)


# ---- 2. row counts: a lone group, a full and a partial wave, a partial last block ------------------
@pytest.fixture(scope="module")
def many(keys, reg):
    i = next(i for i, k in enumerate(keys) if k.name == "openssl_2048")
    msgs = [hashlib.sha256(b"rows-%d" % r).digest() for r in range(257)]
    salts = [hashlib.sha256(b"salt-%d" % r).digest() for r in range(257)]
    return reg[i], msgs, salts, [keys[i].sign(m, s) for m, s in zip(msgs, salts)]


@pytest.mark.parametrize("n", (1, 8, 9, 33, 257))
def test_row_counts(eng, many, n):
    kid, msgs, salts, want = many
    sig, ln, st = device_sign(eng, 64, [kid] * n, msgs[:n], salts[:n])
    assert not st.any()
    assert all(row_is(sig, ln, i, want[i]) for i in range(n))


# ---- 3. the verifiers agree --------------------------------------------------------------------------
def test_verifiers_agree(eng, keys, lanes, signed):
    sig, ln, st = signed
    sigs = [sig[i][:int(ln[i])].tobytes() for i in range(len(lanes))]
    ders = [keys[l["key"]].der() for l in lanes]
    msgs = [l["msg"] for l in lanes]
    gst, _ = eng.verify_batch([RSA] * len(lanes), ders, sigs, msgs, rsa=True)  # K8
    assert not gst.any()
    vid = {}
    try:
        for i, k in enumerate(keys):  # K18, over the modulus the add returned
            vid[i], vst = eng.vkey_add_rsa(bc.encode_key(k.n, k.e))
            assert vst == OK
        kst, _ = eng.rsa_verify_keyed_batch([vid[l["key"]] for l in lanes], sigs, msgs)
        assert not kst.any()
    finally:
        for v in vid.values():
            eng.vkey_remove(v)
    assert all(bc.verify(d, s, m) == OK for d, s, m in zip(ders, sigs, msgs))
    # another message, or one salt bit flipped: another signature, the restatement's
    l = lanes[0]
    k = keys[l["key"]]
    flipped = bytes([l["salt"][0] ^ 1]) + l["salt"][1:]
    other = l["msg"] + b"!"
    s2, l2, st2 = eng.rsa_sign_batch([l["id"]] * 2, [l["msg"], other], [flipped, l["salt"]])
    assert not st2.any()
    assert row_is(s2, l2, 0, k.sign(l["msg"], flipped)) and row_is(s2, l2, 1, k.sign(other, l["salt"]))
    assert len({sigs[0], s2[0][:k.k].tobytes(), s2[1][:k.k].tobytes()}) == 3


# ---- 4. statuses and precedence ----------------------------------------------------------------------
def test_statuses_and_precedence(keys):
    from corda_amd.engine import Engine
    k64 = next(k for k in keys if k.name == "py_1024")
    kgone = next(k for k in keys if k.name == "py_1536_e17")
    assert (k64.words, kgone.words) == (64, 64)  # both fast; the other class below is openssl_3072's
    k3072 = next(k for k in keys if k.name == "openssl_3072")
    msg, salt = b"m" * 32, b"s" * 32
    with Engine(1) as e:
        ed_id, _ = e.signer_add_ed25519(hashlib.sha256(b"ed").digest())
        ec_id, est, _ = e.signer_add_ecdsa(3, (7).to_bytes(32, "big"))
        assert est == OK
        ed_before, _ = e.sign_batch([ed_id], [msg])
        ec_before = e.ecdsa_sign_batch([ec_id], [msg])
        live, st, _ = e.signer_add_rsa(*k64.crt(), k64.e)
        gone, st2, _ = e.signer_add_rsa(*kgone.crt(), kgone.e)
        assert st == OK and st2 == OK
        e.signer_remove(gone)
        reused, st3, _ = e.signer_add_rsa(*k3072.crt(), k3072.e)  # takes the freed slot under a new id
        assert st3 == OK and reused != gone and reused & 4095 == gone & 4095
        never = 4095 | (77 << 12)
        ids = [live, live, gone, reused, ed_id, ec_id, live, never, live, gone]
        msgs = [msg, msg, msg, msg, msg, msg, b"", msg, b"", msg]
        gate = [0, 1, 0, 0, 0, 0, 0, 0, 1, 1]  # a gated lane; gated and empty; gated and removed: SKIPPED first
        want = [OK, SKIPPED, UNKNOWN, OK, UNKNOWN, UNKNOWN, EMPTY, UNKNOWN, SKIPPED, SKIPPED]
        sig, ln, got = e.rsa_sign_batch(ids, msgs, [salt] * len(ids), gate=gate)
        assert [int(x) for x in got] == want
        for i, s in enumerate(want):
            exp = None if s != OK else (k64 if ids[i] == live else k3072).sign(msgs[i], salt)
            assert row_is(sig, ln, i, exp), i
        # the device call, class 64: the 3072-bit key is of another class, the rest as above
        dsig, dln, dst = device_sign(e, 64, ids, [msg] * len(ids), [salt] * len(ids), gate=gate)
        assert [int(x) for x in dst] == [OK, SKIPPED, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN, OK, UNKNOWN, SKIPPED, SKIPPED]
        for i, s in enumerate(dst):
            assert row_is(dsig, dln, i, k64.sign(msg, salt) if s == OK else None), i
        # ... and class 96 takes it and none of the others; msg_len 0: EMPTY for the ungated live lane
        dsig, dln, dst = device_sign(e, 96, ids, [msg] * len(ids), [salt] * len(ids), gate=gate)
        assert [int(x) for x in dst] == [UNKNOWN, SKIPPED, UNKNOWN, OK, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN, SKIPPED,
                                         SKIPPED]
        assert row_is(dsig, dln, 3, k3072.sign(msg, salt)) and not dsig[[0, 1, 2, 4, 5, 6, 7, 8, 9]].any()
        zsig, zln, zst = device_sign(e, 64, ids, [b""] * len(ids), [salt] * len(ids), gate=gate, msg_len=0)
        assert [int(x) for x in zst] == [EMPTY, SKIPPED, UNKNOWN, UNKNOWN, UNKNOWN, UNKNOWN, EMPTY, UNKNOWN, SKIPPED,
                                         SKIPPED]
        assert not zsig.any() and not zln.any()
        # the reverse: an RSA id is no Ed25519 and no ECDSA signer, and theirs still sign as before
        s1, st1 = e.sign_batch([live, ed_id], [msg, msg])
        assert [int(x) for x in st1] == [UNKNOWN, OK] and not s1[0].any() and (s1[1] == ed_before[0]).all()
        s2, l2, st2 = e.ecdsa_sign_batch([live, ec_id, reused], [msg] * 3)
        assert [int(x) for x in st2] == [UNKNOWN, OK, UNKNOWN] and not s2[0].any() and not s2[2].any()
        assert (s2[1] == ec_before[0][0]).all() and l2[1] == ec_before[1][0]
        # a NULL salt, and offsets that run backwards: INVALID_ARG with the outputs untouched
        from corda_amd import _lib
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        idv, mo = np.array([live], np.uint32), np.array([0, 32], np.uint64)
        mb, sa = np.frombuffer(msg, np.uint8).copy(), np.frombuffer(salt, np.uint8).copy()
        osig, olen, ost = np.full(512, 0xA5, np.uint8), np.full(1, 0xA5A5, np.uint16), np.full(1, 0xA5, np.uint8)
        for b in (_lib.RsaSignBatch(1, p(idv), p(mb), p(mo), None, None, p(osig), p(olen), p(ost), 32),
                  _lib.RsaSignBatch(1, p(idv), p(mb), p(np.array([32, 0], np.uint64)), None, p(sa), p(osig), p(olen),
                                    p(ost), 32)):
            assert _lib.lib().cordahip_rsa_sign(e._ctx, ctypes.byref(b)) == _lib.ERR_INVALID_ARG
            assert (osig == 0xA5).all() and olen[0] == 0xA5A5 and ost[0] == 0xA5


# ---- 5. registration ---------------------------------------------------------------------------------
def test_registration(keys):
    from corda_amd import _lib
    from corda_amd.engine import Engine
    k = next(k for k in keys if k.name == "py_1024")
    msg, salt = b"r" * 32, b"t" * 32
    with Engine(1) as e:
        # device calls before any RSA key: UNKNOWN_KEY for every lane, and nothing of the table exists
        base = e.device_mem(0)[0]
        for w in (64, 96, 128):
            sig, ln, st = device_sign(e, w, [1, 4097, 0], [msg] * 3, [salt] * 3)
            assert (st == UNKNOWN).all() and not sig.any() and not ln.any()
        hsig, hln, hst = e.rsa_sign_batch([1, 4097], [msg] * 2, [salt] * 2)
        assert (hst == UNKNOWN).all() and not hsig.any() and not hln.any()
        e.trim()
        assert e.device_mem(0)[0] == base
        # every rejected key: data, no slot, no memory
        for kk in (k, next(x for x in keys if x.name == "openssl_3072")):
            for what, comp, ee, want in model.rejected_keys(kk):
                if any(c is None for c in comp):  # a zero-length component: only the C call can say it
                    parts = [b"" if c is None else c.to_bytes(max((c.bit_length() + 7) // 8, 1), "big") for c in comp]
                    key = _lib.RsaPrivateKey(*parts, *[len(x) for x in parts], ee)
                    kid, st, ml = ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint32()
                    mod = ctypes.create_string_buffer(512)
                    assert _lib.lib().cordahip_signer_add_rsa(e._ctx, ctypes.byref(key), ctypes.byref(kid),
                                                              ctypes.byref(st), mod, ctypes.byref(ml)) == 0
                    got = (kid.value, st.value)
                else:
                    got = e.signer_add_rsa(*comp, ee)[:2]
                assert got == (NO_ID, bc.BAD_KEY if want == "consistency" else want), (kk.name, what)
        for kk in model.private_keys():
            if kk.name in model.DECLINED:
                assert e.signer_add_rsa(*kk.crt(), kk.e) == (NO_ID, bc.UNSUPPORTED, None), kk.name
        assert e.device_mem(0)[0] == base  # also after the consistency runs: their table went with them
        # the table is made by the first add that is accepted, and no slot was taken before it
        first, st, mod = e.signer_add_rsa(*k.crt(), k.e)
        assert st == OK and first & 4095 == 0 and mod == k.n.to_bytes(k.k, "big")
        assert e.device_mem(0)[0] - base == _lib.RSA_SIGN_TABLE_BYTES
        ids = [first] + [e.signer_add_rsa(*k.crt(), k.e)[0] for _ in range(_lib.RSA_SIGNER_MAX_KEYS - 1)]
        assert len(set(ids)) == 64 and NO_ID not in ids
        assert e.device_mem(0)[0] - base == _lib.RSA_SIGN_TABLE_BYTES
        with pytest.raises(_lib.EngineError) as err:  # the 65th
            e.signer_add_rsa(*k.crt(), k.e)
        assert err.value.code == _lib.ERR_OUT_OF_MEMORY
        ed_id, _ = e.signer_add_ed25519(hashlib.sha256(b"next to 64 RSA keys").digest())  # the pool is not full
        e.signer_remove(ids[17])
        again, st, _ = e.signer_add_rsa(*k.crt(), k.e)
        assert st == OK and again not in ids and again & 4095 == ids[17] & 4095
        sig, ln, st = e.rsa_sign_batch([ids[0], ids[17], again, ids[63]], [msg] * 4, [salt] * 4)
        assert [int(x) for x in st] == [OK, UNKNOWN, OK, OK]
        want = k.sign(msg, salt)
        assert row_is(sig, ln, 0, want) and row_is(sig, ln, 1, None) and row_is(sig, ln, 2, want) and row_is(sig, ln, 3, want)
        e.trim()
        assert e.device_mem(0)[0] - base >= _lib.RSA_SIGN_TABLE_BYTES  # kept (with the Ed25519 signer's)


def test_table_made_by_first_accepted_add(keys):
    from corda_amd import _lib
    from corda_amd.engine import Engine
    k = next(k for k in keys if k.name == "py_1024")
    with Engine(1) as e:
        base = e.device_mem(0)[0]
        # declined on the host: nothing reaches a device
        assert e.signer_add_rsa(k.p + 1, k.q, k.dp, k.dq, k.qinv, k.e)[:2] == (NO_ID, bc.BAD_KEY)
        big = next(x for x in model.private_keys() if x.name == "py_4104")
        assert e.signer_add_rsa(*big.crt(), big.e)[:2] == (NO_ID, bc.UNSUPPORTED)
        assert e.device_mem(0)[0] == base
        kid, st, _ = e.signer_add_rsa(*k.crt(), k.e)
        assert st == OK and e.device_mem(0)[0] - base == _lib.RSA_SIGN_TABLE_BYTES
        e.signer_remove(kid)
        assert e.device_mem(0)[0] - base == _lib.RSA_SIGN_TABLE_BYTES
        sig, ln, st = e.rsa_sign_batch([kid], [b"x"], [bytes(32)])
        assert st[0] == UNKNOWN and row_is(sig, ln, 0, None)


# ---- 6. chunking and tickets -------------------------------------------------------------------------
def test_three_chunks_classes_interleaved(eng, keys, lanes, signed, monkeypatch):
    by_class = [[l for l in lanes if keys[l["key"]].words == w] for w in (64, 96, 128)]
    # 50 lanes a class, interleaved: three chunks of 64, 64 and 22
    order = [c[r % len(c)] for r in range(50) for c in by_class]
    assert len(order) == 150
    args = ([l["id"] for l in order], [l["msg"] for l in order], [l["salt"] for l in order])
    gate = [int(i % 11 == 5) for i in range(len(order))]
    one = eng.rsa_sign_batch(*args, gate=gate)
    monkeypatch.setenv("CORDAHIP_HOST_CHUNK", "64")
    three = eng.rsa_sign_batch(*args, gate=gate)
    ticket = eng.rsa_sign_batch(*args, gate=gate, async_=True).wait()
    for got in (three, ticket):
        assert all((a == b).all() for a, b in zip(one, got))
    sig, ln, st = one
    for i, l in enumerate(order):
        assert st[i] == (SKIPPED if gate[i] else OK) and row_is(sig, ln, i, None if gate[i] else l["want"]), i


# ---- 7. a gate written on the same stream ------------------------------------------------------------
def test_device_chain_commit_then_sign(eng, keys, reg):
    """commit -> sign on one stream with no host round trip: the tx_status cordahip_commit_inputs_device
    writes is the RSA signer's gate."""
    import torch
    import commit_log_worker as W
    from corda_amd import _lib
    dev = torch.device("cuda:0")
    i = next(i for i, k in enumerate(keys) if k.name == "openssl_2048_b")
    k, kid = keys[i], reg[i]
    lid = eng.commit_log_create(10)
    try:
        now, tol = 10**18, 10**9
        txs = [(W.h("rtx", 0), 7, [W.ref(0), W.ref(1)], None),
               (W.h("rtx", 1), 8, [W.ref(1)], None),                    # conflict with the one before it
               (W.h("rtx", 2), 8, [W.ref(2)], (None, now - tol - 1)),   # out of window
               (W.h("rtx", 3), 8, [W.ref(3)], None)]
        n = len(txs)
        flat = [r for tx in txs for r in tx[2]]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(tx[2]) for tx in txs])
        absent = _lib.TW_SIDE_ABSENT
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_txid = to(np.frombuffer(b"".join(tx[0] for tx in txs), np.uint8).reshape(n, 32).copy())
        d_caller = to(np.array([tx[1] for tx in txs], np.int32))
        d_refs = to(eng._state_refs(flat).view(np.uint8).reshape(-1, 36)[:len(flat)].copy())
        d_from = to(np.array([absent if not tx[3] or tx[3][0] is None else tx[3][0] for tx in txs], np.int64))
        d_until = to(np.array([absent if not tx[3] or tx[3][1] is None else tx[3][1] for tx in txs], np.int64))
        d_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_cm = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_rs = torch.full((len(flat),), 0xA5, dtype=torch.uint8, device=dev)
        d_rb = torch.full((len(flat), 40), 0xA5, dtype=torch.uint8, device=dev)
        d_kid = to(np.full(n, kid, np.int64).astype(np.uint32).view(np.int32))
        salts = [model.salt(900 + t) for t in range(n)]
        d_salt = to(np.frombuffer(b"".join(salts), np.uint8).reshape(n, 32).copy())
        d_sig = torch.full((n, 4 * k.words), 0xA5, dtype=torch.uint8, device=dev)
        d_len = torch.full((n,), -1, dtype=torch.int16, device=dev)
        d_sst = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            eng.commit_inputs_device(lid, d_txid, d_caller, d_refs, to(off), d_st, d_cm, d_rs, d_rb, tw_from=d_from,
                                     tw_until=d_until, now_ns=now, tolerance_ns=tol, stream=stream)
            eng.rsa_sign_keyed_device(d_kid, d_txid, d_salt, d_sig, d_len, d_sst, gate=d_st, stream=stream)
        stream.synchronize()
        assert [int(x) for x in d_st.cpu().numpy()] == [OK, _lib.COMMIT_CONFLICT, _lib.COMMIT_TIME_WINDOW_INVALID, OK]
        sig, ln, sst = d_sig.cpu().numpy(), d_len.cpu().numpy().view(np.uint16), d_sst.cpu().numpy()
        assert [int(x) for x in sst] == [OK, SKIPPED, SKIPPED, OK]
        for t, tx in enumerate(txs):
            assert row_is(sig, ln, t, k.sign(tx[0], salts[t]) if sst[t] == OK else None), t
    finally:
        eng.commit_log_destroy(lid)


def test_sign_with_rsa_key_through_resolve(eng, keys, reg):
    """resolve._sign_with with an RSA signer id: the caller's salts give the restatement's bytes, drawn
    salts give signatures the verifier takes"""
    from corda_amd import resolve as R
    i = next(i for i, k in enumerate(keys) if k.name == "py_2049")
    k, kid = keys[i], reg[i]
    ids = [hashlib.sha256(b"root-%d" % t).digest() for t in range(5)]
    salts = [model.salt(300 + t) for t in range(5)]
    sigs, st = R._sign_with(eng, kid, ids, [0, 0, 1, 0, 0], salts=salts)
    assert [int(x) for x in st] == [OK, OK, SKIPPED, OK, OK]
    assert [s for t, s in enumerate(sigs) if t != 2] == [k.sign(m, s) for t, (m, s) in enumerate(zip(ids, salts)) if t != 2]
    drawn, st = R._sign_with(eng, kid, ids, None)
    assert not st.any() and all(bc.verify(k.der(), s, m) == OK for s, m in zip(drawn, ids))
    assert all(a != b for a, b in zip(drawn, sigs))


# ---- 8. more than one device ---------------------------------------------------------------------------
def test_three_device_replicas(keys, lanes, monkeypatch):
    """The shard split and the per-device tables on a context of three Device objects
    (CORDAHIP_TEST_DEVICE_REPLICAS): lanes sharded over the devices give the single-device bytes; add
    and remove reach every replica."""
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_TEST_DEVICE_REPLICAS", "3")
    use = [i for i, k in enumerate(keys) if k.name in ("py_1024", "openssl_2048", "py_1536_e17", "py_3071")]
    with Engine(1) as e:
        assert e.device_count() == 3
        kid = {}
        for i in use:
            kid[i], st, mod = e.signer_add_rsa(*keys[i].crt(), keys[i].e)
            assert st == OK and mod == keys[i].n.to_bytes(keys[i].k, "big")
        rows = [l for l in lanes if l["key"] in use]
        rows = (rows * 9)[:200]  # shards of 128 and 72 lanes, the third empty
        sig, ln, st = e.rsa_sign_batch([kid[l["key"]] for l in rows], [l["msg"] for l in rows], [l["salt"] for l in rows])
        assert not st.any() and all(row_is(sig, ln, i, l["want"]) for i, l in enumerate(rows))
        l = next(l for l in lanes if l["key"] == use[0] and len(l["msg"]) == 32)
        for dev in range(3):
            dsig, dln, dst = device_sign(e, 64, [kid[use[0]]], [l["msg"]], [l["salt"]], device=dev)
            assert dst[0] == OK and row_is(dsig, dln, 0, l["want"]), dev
        e.signer_remove(kid[use[0]])
        for dev in range(3):
            dsig, dln, dst = device_sign(e, 64, [kid[use[0]]], [l["msg"]], [l["salt"]], device=dev)
            assert dst[0] == UNKNOWN and row_is(dsig, dln, 0, None), dev
