"""Ed25519 verification against registered public keys on the GPU (K12:
cordahip_vkey_add_ed25519, cordahip_vkey_remove, cordahip_verify_keyed,
cordahip_verify_keyed_submit, cordahip_ed25519_verify_keyed_device) against
tests/golden/ed25519_vectors.json and the C oracle, lane for lane. Outputs are prefilled
with 0xA5 and sit between guard bytes, so a lane the library does not write, or a write
outside the arrays, shows."""
import collections
import ctypes
import hashlib

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd._lib import lib

pytestmark = pytest.mark.gpu
OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, EMPTY = _lib.OK, 1, 2, 3, _lib.EMPTY
UNKNOWN = _lib.VERIFY_UNKNOWN_KEY
GUARD = 64
# ed25519_vkey.hpp: 64 tables of 512 KiB and the base point's, 64 records of 64 bytes, 64 bytes of scratch
VKEY_BYTES = 65 * 512 * 1024 + 64 * 64 + 64


def csign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


def oracle_statuses(oracle, pubs, sigs, msgs):
    """oracle_ed25519_verify_batch over dense rows (doVerify rules)."""
    n = len(pubs)
    k = np.frombuffer(b"".join(pubs), np.uint8).copy()
    s = np.frombuffer(b"".join(sigs), np.uint8).copy()
    ml = len(msgs[0])
    m = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()
    want = np.zeros(n, np.uint8)
    oracle.oracle_ed25519_verify_batch(n, k.ctypes.data, s.ctypes.data, m.ctypes.data, ml, want.ctypes.data, 8)
    return want


def verdict_bits(verdict, n):
    return np.array([(int(verdict[i >> 6]) >> (i & 63)) & 1 for i in range(n)], np.uint8)


class HostBatch:
    """cordahip_keyed_sig_batch arrays with guard bytes around status and verdict, everything 0xA5."""

    def __init__(self, ids, sigs, msgs, flags=0):
        self.n = n = len(sigs)
        self.flags = flags
        self.ids = np.asarray(ids, np.uint32)
        self.soff = np.zeros(n + 1, np.uint64)
        self.soff[1:] = np.cumsum([len(s) for s in sigs])
        self.sig = np.frombuffer(b"".join(sigs) or b"\0", np.uint8).copy()
        self.moff = np.zeros(n + 1, np.uint64)
        self.moff[1:] = np.cumsum([len(m) for m in msgs])
        self.msg = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()
        self.words = (n + 63) // 64
        self.st_buf = np.full(GUARD + n + GUARD, 0xA5, np.uint8)
        self.vd_buf = np.full(GUARD + self.words * 8 + GUARD, 0xA5, np.uint8)

    def batch(self, soff=None, moff=None, sig_bytes=None, msg_bytes=None, verdict=True):
        p = lambda a: a.ctypes.data  # noqa: E731
        return _lib.KeyedSigBatch(self.n, p(self.ids), p(self.sig), p(self.soff if soff is None else soff),
                                  p(self.msg), p(self.moff if moff is None else moff), p(self.st_buf) + GUARD,
                                  p(self.vd_buf) + GUARD if verdict else None, self.flags,
                                  int(self.soff[self.n]) if sig_bytes is None else sig_bytes,
                                  int(self.moff[self.n]) if msg_bytes is None else msg_bytes)

    @property
    def st(self):
        return self.st_buf[GUARD:GUARD + self.n]

    @property
    def verdict(self):
        return self.vd_buf[GUARD:GUARD + self.words * 8].view(np.uint64)

    def untouched(self):
        return (self.st_buf == 0xA5).all() and (self.vd_buf == 0xA5).all()

    def guards_intact(self):
        return all((b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all() for b in (self.st_buf, self.vd_buf))

    def run(self, engine, verdict=True):
        rc = lib().cordahip_verify_keyed(engine.ctx, ctypes.byref(self.batch(verdict=verdict)))
        assert rc == 0, rc
        assert self.guards_intact()
        if not verdict:  # a NULL verdict pointer: statuses only
            assert (self.vd_buf == 0xA5).all()
            return self.st.copy()
        # the verdict bit is status == OK, the bits past n are zero
        bits = verdict_bits(self.verdict, self.words * 64)
        assert np.array_equal(bits[:self.n], (self.st == OK).astype(np.uint8)) and not bits[self.n:].any()
        return self.st.copy()


@pytest.fixture(scope="module")
def five(engine, oracle):
    """Five keys registered on the session engine: ([ids], [seeds], [pubs])."""
    seeds = [hashlib.sha256(b"vkey-seed-%d" % i).digest() for i in range(5)]
    pubs = [csign(oracle, s, b"x")[0] for s in seeds]
    ids = []
    for p in pubs:
        kid, st = engine.vkey_add_ed25519(p)
        assert st == OK and kid != _lib.VKEY_NO_ID
        ids.append(kid)
    assert len(set(ids)) == 5
    yield ids, seeds, pubs
    for kid in ids:
        engine.vkey_remove(kid)


# ---- 1. golden vectors -------------------------------------------------------------
def test_golden_vectors_host_call(ed_vectors, oracle):
    from corda_amd.engine import Engine
    assert len(ed_vectors) == 483
    left_out = [v for v in ed_vectors if len(v["pub"]) != 32]
    vecs = [v for v in ed_vectors if len(v["pub"]) == 32]
    assert len(left_out) == 2 and all(v["cat"] == "key_len" and len(v["pub"]) == 31 for v in left_out)
    assert len(vecs) == 481
    keys = list(dict.fromkeys(v["pub"] for v in vecs))
    assert len(keys) == 269
    by_key = collections.defaultdict(list)
    for v in vecs:
        by_key[v["pub"]].append(v)
    bad_keys, registered, all_ids = 0, 0, set()
    ran = collections.Counter()
    accepted = collections.Counter()
    with Engine(1) as eng:
        for g in range(0, len(keys), _lib.VKEY_MAX_KEYS):
            group = keys[g:g + _lib.VKEY_MAX_KEYS]
            ids = {}
            for k in group:
                kid, st = eng.vkey_add_ed25519(k)
                if st == BAD_KEY:
                    assert kid == _lib.VKEY_NO_ID
                    assert all(v["status"] == BAD_KEY for v in by_key[k]), k.hex()
                    bad_keys += 1
                    continue
                assert st == OK and kid not in all_ids
                all_ids.add(kid)
                ids[k] = kid
                registered += 1
            lanes = [v for k in group if k in ids for v in by_key[k]]
            lane_ids = [ids[v["pub"]] for v in lanes]
            got = HostBatch(lane_ids, [v["sig"] for v in lanes], [v["msg"] for v in lanes]).run(eng)
            wrong = [(v["cat"], v["note"], int(s), v["status"]) for v, s in zip(lanes, got) if s != v["status"]]
            assert not wrong, wrong[:10]
            got_iv = HostBatch(lane_ids, [v["sig"] for v in lanes], [v["msg"] for v in lanes],
                               flags=_lib.FLAG_IS_VALID).run(eng)
            want_iv = [oracle.oracle_ed25519_is_valid(v["pub"], 32, v["sig"], len(v["sig"]), v["msg"], len(v["msg"]))
                       for v in lanes]
            wrong = [(v["cat"], v["note"], int(s), w) for v, s, w in zip(lanes, got_iv, want_iv) if s != w]
            assert not wrong, wrong[:10]
            for v in lanes:
                ran[v["cat"]] += 1
                accepted[v["cat"]] += v["status"] == OK
            for kid in ids.values():  # the next group takes these slots under new ids
                eng.vkey_remove(kid)
    assert bad_keys == 28 and registered == 241
    # the lanes where a table can go wrong were in the run, and the signature shapes too
    assert ran["key_small_order"] == 8 and ran["key_identity_signbit"] == 8 and ran["key_mixed_order"] == 34, ran
    assert accepted["key_identity_signbit"] == 8 and accepted["key_mixed_order"] > 0, accepted
    assert accepted["key_noncanonical_y"] > 0, accepted
    assert ran["s_plus_kL"] == 146 and ran["sig_len"] == 2 and ran["empty"] == 3 and ran["long_msg"] == 10, ran
    assert {len(v["sig"]) for v in vecs} == {0, 10, 63, 64, 65} and max(len(v["msg"]) for v in vecs) == 1000


# ---- 2. seeded corruption against the oracle -----------------------------------------
KINDS = ["bit_flip", "other_key_id", "s_bit_255", "s_random"]


def test_seeded_corruption_matches_oracle_and_generic_path(engine, oracle, five):
    ids, seeds, pubs = five
    n = 4096
    rng = np.random.default_rng(20261019)
    lane_id, lane_pub, sigs, msgs, kind = [], [], [], [], []
    for i in range(n):
        k = i % 5
        msg = hashlib.sha256(b"vkey-lane-%d" % i).digest()
        sig = bytearray(csign(oracle, seeds[k], msg)[1])
        use = k
        kd = None
        if i % 4 == 3:
            kd = KINDS[(i // 4) % 4]
            if kd == "bit_flip":
                bit = int(rng.integers(0, 512))
                sig[bit >> 3] ^= 1 << (bit & 7)
            elif kd == "other_key_id":
                use = (k + 1 + int(rng.integers(0, 4))) % 5
            elif kd == "s_bit_255":
                sig[63] |= 0x80
            else:
                sig[32:] = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        lane_id.append(ids[use])
        lane_pub.append(pubs[use])
        sigs.append(bytes(sig))
        msgs.append(msg)
        kind.append(kd)
    want = oracle_statuses(oracle, lane_pub, sigs, msgs)
    got = HostBatch(lane_id, sigs, msgs).run(engine)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), kind[i], int(got[i]), int(want[i])) for i in bad[:10]]
    gen, _ = engine.ed25519_verify_host(np.frombuffer(b"".join(lane_pub), np.uint8),
                                        np.frombuffer(b"".join(sigs), np.uint8),
                                        np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32))
    assert np.array_equal(gen, got)
    assert (got == OK).sum() > n // 2 and (got == BAD_SIG).any() and set(got.tolist()) == {OK, BAD_SIG}
    assert all(got[i] == OK for i in range(n) if kind[i] is None)
    for kd in KINDS:
        st = {int(want[i]) for i in range(n) if kind[i] == kd}
        assert BAD_SIG in st, kd  # every kind rejects; a kind the oracle also accepts was matched above


# ---- 3. the device call ----------------------------------------------------------------
@pytest.mark.parametrize("msg_len", [32, 200, 0])
def test_device_call_partial_wave_and_unknown_ids(engine, oracle, five, msg_len):
    import torch
    ids, seeds, pubs = five
    n = 2085  # not a multiple of 64 or 256: a partial last wave and a partial verdict word
    words = (n + 63) // 64
    removed, st = engine.vkey_add_ed25519(pubs[0])
    assert st == OK
    engine.vkey_remove(removed)
    never = (removed & 63) | (0x155555 << 6)
    unknown_ids = {7: never, 64: _lib.VKEY_NO_ID, 1000: removed, n - 1: never}
    lane_id, lane_pub, sigs, msgs = [], [], [], []
    for i in range(n):
        k = i % 5
        msg = hashlib.sha512(b"vkey-dev-%d" % i).digest() * 4
        msg = msg[:msg_len]
        sig = bytearray(csign(oracle, seeds[k], msg)[1]) if msg_len else bytearray(b"\x01" * 64)
        if i % 7 == 3:
            sig[i % 64] ^= 1 << (i % 8)
        lane_id.append(unknown_ids.get(i, ids[k]))
        lane_pub.append(pubs[k])
        sigs.append(bytes(sig))
        msgs.append(msg)
    want = oracle_statuses(oracle, lane_pub, sigs, msgs)
    for i in unknown_ids:
        want[i] = UNKNOWN
    if msg_len == 0:
        assert all(want[i] == EMPTY for i in range(n) if i not in unknown_ids)
    else:
        assert (want == OK).sum() > n // 2 and (want == BAD_SIG).sum() > n // 10
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    pad = 100
    with torch.cuda.stream(stream):
        t_ids = torch.from_numpy(np.asarray(lane_id, np.uint32).view(np.int32).copy()).to(dev)
        t_sig = torch.from_numpy(np.frombuffer(b"".join(sigs), np.uint8).reshape(n, 64).copy()).to(dev)
        t_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).reshape(n, msg_len).copy()).to(dev) \
            if msg_len else torch.empty((n, 0), dtype=torch.uint8, device=dev)
        t_st = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=dev)
        t_vd = torch.full((2 + words + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
        engine.ed25519_verify_keyed_device(t_ids, t_sig, t_msg, t_st[pad:pad + n], t_vd[2:2 + words], stream=stream)
    stream.synchronize()
    st_all, vd_all = t_st.cpu().numpy(), t_vd.cpu().numpy().view(np.uint64)
    assert (st_all[:pad] == 0xA5).all() and (st_all[pad + n:] == 0xA5).all()  # guards, and the rows after n
    assert (vd_all[:2] == 0xA5A5A5A5A5A5A5A5).all() and (vd_all[2 + words:] == 0xA5A5A5A5A5A5A5A5).all()
    got = st_all[pad:pad + n]
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), int(got[i]), int(want[i])) for i in bad[:10]]
    bits = verdict_bits(vd_all[2:2 + words], words * 64)
    assert np.array_equal(bits[:n], (want == OK).astype(np.uint8)) and not bits[n:].any()
    assert all(bits[i] == 0 for i in unknown_ids)


# ---- 4. registry lifecycle ---------------------------------------------------------------
def test_registry_lifecycle(oracle):
    from corda_amd.engine import Engine
    seeds = [hashlib.sha256(b"vkey-life-%d" % i).digest() for i in range(3)]
    pubs = [csign(oracle, s, b"x")[0] for s in seeds]
    msg = hashlib.sha256(b"vkey-life-msg").digest()
    sig = [csign(oracle, s, msg)[1] for s in seeds]

    def mem(e):
        u = ctypes.c_uint64()
        assert lib().cordahip_device_mem(e.ctx, 0, ctypes.byref(u), None, None) == 0
        return u.value

    with Engine(1) as e:
        # no key yet: every id is unknown
        assert HostBatch([0, 64], [sig[0]] * 2, [msg] * 2).run(e).tolist() == [UNKNOWN] * 2
        assert lib().cordahip_trim(e.ctx) == 0  # the call's staging released: the account is at rest
        before = mem(e)
        a, st = e.vkey_add_ed25519(pubs[0])
        assert st == OK
        assert mem(e) - before == VKEY_BYTES  # the tables appear with the first add ...
        assert HostBatch([a], [sig[0]], [msg]).run(e).tolist() == [OK]
        assert lib().cordahip_trim(e.ctx) == 0
        assert mem(e) - before == VKEY_BYTES  # ... and survive trim, which takes the staging alone
        assert HostBatch([a], [sig[0]], [msg]).run(e).tolist() == [OK]
        b, st = e.vkey_add_ed25519(pubs[0])  # the same bytes again: another id
        assert st == OK and b != a
        assert HostBatch([a, b], [sig[0]] * 2, [msg] * 2).run(e).tolist() == [OK, OK]
        e.vkey_remove(a)
        assert lib().cordahip_vkey_remove(e.ctx, a) == _lib.ERR_INVALID_ARG  # not live any more
        assert HostBatch([a, b], [sig[0]] * 2, [msg] * 2).run(e).tolist() == [UNKNOWN, OK]
        c, st = e.vkey_add_ed25519(pubs[1])  # takes the freed slot under a new id
        assert st == OK and c != a and (c & 63) == (a & 63)
        assert HostBatch([c, c, a], [sig[1], sig[0], sig[0]], [msg] * 3).run(e).tolist() == [OK, BAD_SIG, UNKNOWN]
        # fill the registry
        rest = []
        while True:
            kid = ctypes.c_uint32(123)
            kst = ctypes.c_uint8(0xA5)
            rc = lib().cordahip_vkey_add_ed25519(e.ctx, pubs[2], ctypes.byref(kid), ctypes.byref(kst))
            if rc != 0:
                break
            assert kst.value == OK
            rest.append(kid.value)
            assert len(rest) <= _lib.VKEY_MAX_KEYS
        assert rc == _lib.ERR_OUT_OF_MEMORY and len(rest) == _lib.VKEY_MAX_KEYS - 2
        assert len(set(rest + [b, c])) == _lib.VKEY_MAX_KEYS
        lanes = [b, c, rest[0], rest[-1]]
        assert HostBatch(lanes, [sig[0], sig[1], sig[2], sig[2]], [msg] * 4).run(e).tolist() == [OK] * 4
        assert mem(e) - before >= VKEY_BYTES and mem(e) - before < VKEY_BYTES + (8 << 20)
        # a key that does not decode takes no slot and is no error ...
        e.vkey_remove(rest.pop())
        bad = bytes([2] + [0] * 31)  # y = 2 is not on the curve
        assert oracle.oracle_ed25519_verify(bad, 32, sig[0], 64, msg, 32) == BAD_KEY
        assert e.vkey_add_ed25519(bad) == (_lib.VKEY_NO_ID, BAD_KEY)
        d, st = e.vkey_add_ed25519(pubs[2])  # ... the free slot is still there
        assert st == OK
        assert lib().cordahip_vkey_remove(e.ctx, _lib.VKEY_NO_ID) == _lib.ERR_INVALID_ARG


# ---- 5. bad CSR --------------------------------------------------------------------------
def test_bad_csr_is_invalid_arg_and_leaves_outputs(engine, oracle, five):
    ids, seeds, _ = five
    n = 70
    msgs = [hashlib.sha256(b"vkey-csr-%d" % i).digest() for i in range(n)]
    sigs = [csign(oracle, seeds[i % 5], msgs[i])[1] for i in range(n)]
    lane_id = [ids[i % 5] for i in range(n)]

    def decreasing(off):
        o = off.copy()
        o[30] = o[31] + 1
        return o

    def past_end(off):
        o = off.copy()
        o[n] += 1
        return o

    for which, mutate in [("soff", decreasing), ("soff", past_end), ("moff", decreasing), ("moff", past_end)]:
        hb = HostBatch(lane_id, sigs, msgs)
        bad = mutate(getattr(hb, which))
        rc = lib().cordahip_verify_keyed(engine.ctx, ctypes.byref(hb.batch(**{which: bad})))
        assert rc == _lib.ERR_INVALID_ARG, (which, mutate.__name__)
        assert hb.untouched(), (which, mutate.__name__)
        t = ctypes.c_uint64()
        assert lib().cordahip_verify_keyed_submit(engine.ctx, ctypes.byref(hb.batch(**{which: bad})),
                                                  ctypes.byref(t)) == 0
        assert lib().cordahip_wait(engine.ctx, t.value, -1) == _lib.ERR_INVALID_ARG and hb.untouched()
        assert not HostBatch(lane_id, sigs, msgs).run(engine).any()  # the context is still usable
    hb = HostBatch(lane_id, sigs, msgs, flags=4)  # an unknown flag
    assert lib().cordahip_verify_keyed(engine.ctx, ctypes.byref(hb.batch())) == _lib.ERR_INVALID_ARG and hb.untouched()


# ---- 6. tickets --------------------------------------------------------------------------
def test_two_tickets_waited_in_reverse(engine, oracle, five):
    ids, seeds, pubs = five
    batches = []
    for b, n in enumerate((300, 131)):
        msgs = [hashlib.sha256(b"vkey-ticket-%d-%d" % (b, i)).digest()[:32 - 5 * b] for i in range(n)]
        sigs = [bytearray(csign(oracle, seeds[(i + b) % 5], msgs[i])[1]) for i in range(n)]
        for i in range(b, n, 3):
            sigs[i][40] ^= 4
        sigs = [bytes(s) for s in sigs]
        want = oracle_statuses(oracle, [pubs[(i + b) % 5] for i in range(n)], sigs, msgs)
        assert (want == OK).any() and (want == BAD_SIG).any()
        batches.append(([ids[(i + b) % 5] for i in range(n)], sigs, msgs, want))
    tickets = [engine.verify_keyed_batch(x[0], x[1], x[2], async_=True) for x in batches]
    for t, x in reversed(list(zip(tickets, batches))):
        st, vd = t.wait()
        assert np.array_equal(st, x[3])
        assert np.array_equal(verdict_bits(vd, len(st)), (x[3] == OK).astype(np.uint8))


# ---- 7. the notary client's check ----------------------------------------------------------
def test_validate_notary_signatures(engine, oracle, five):
    from corda_amd import resolve
    ids, seeds, _ = five
    n = 64
    txids = [hashlib.sha256(b"vkey-notary-%d" % i).digest() for i in range(n)]
    sigs = [csign(oracle, seeds[0], t)[1] for t in txids]
    sigs[17] = csign(oracle, seeds[1], txids[17])[1]  # signed by another key
    sigs[40] = sigs[40][:63]                          # truncated
    out = resolve.validate_notary_signatures(engine, ids[0], txids, sigs)
    assert len(out) == n
    assert all(o is None for i, o in enumerate(out) if i not in (17, 40))
    assert isinstance(out[17], resolve.SignatureException) and "Verification failed" in str(out[17])
    assert isinstance(out[40], resolve.SignatureException) and "decoding" in str(out[40])
    never = (ids[0] & 63) | (0x2AAAAA << 6)
    out = resolve.validate_notary_signatures(engine, never, txids[:3], sigs[:3])
    assert all(isinstance(o, resolve.NoSuchElementException) for o in out)
    assert resolve.validate_notary_signatures(engine, ids[0], [], []) == []


# ---- 8. several devices, several chunks -----------------------------------------------------
def test_three_device_replicas_and_chunks(oracle, monkeypatch):
    """The shard split (whole verdict words per device), the chunk loop and the per-device key
    tables on a context of three Device objects (CORDAHIP_TEST_DEVICE_REPLICAS, read by
    cordahip_init): every replica holds the same tables; add and remove reach all of them."""
    import torch
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_TEST_DEVICE_REPLICAS", "3")
    monkeypatch.setenv("CORDAHIP_HOST_CHUNK", "64")
    seeds = [hashlib.sha256(b"vkey-replica-%d" % i).digest() for i in range(3)]
    pubs = [csign(oracle, s, b"x")[0] for s in seeds]
    with Engine(1) as eng:
        assert eng.device_count() == 3
        ids = []
        for p in pubs:
            kid, st = eng.vkey_add_ed25519(p)
            assert st == OK
            ids.append(kid)
        n = 300  # shards of 128, 128 and 44 lanes, chunks of 64
        lens = [32 if i < 150 else 1 + i % 90 for i in range(n)]  # dense chunks, then CSR chunks
        msgs = [(hashlib.sha512(b"vkey-replica-msg-%d" % i).digest() * 2)[:lens[i]] for i in range(n)]
        sigs = [bytearray(csign(oracle, seeds[i % 3], msgs[i])[1]) for i in range(n)]
        for i in range(0, n, 5):
            sigs[i][i % 64] ^= 0x10
        sigs = [bytes(s) for s in sigs]
        want = np.array([oracle.oracle_ed25519_verify(pubs[i % 3], 32, sigs[i], 64, msgs[i], len(msgs[i]))
                         for i in range(n)], np.uint8)
        assert (want == OK).sum() == n - n // 5 and (want == BAD_SIG).sum() == n // 5
        lane_ids = [ids[i % 3] for i in range(n)]
        assert np.array_equal(HostBatch(lane_ids, sigs, msgs).run(eng), want)
        eng.vkey_remove(ids[1])
        got = HostBatch(lane_ids, sigs, msgs).run(eng)
        assert np.array_equal(got, np.where(np.arange(n) % 3 == 1, UNKNOWN, want))
        dev = torch.device("cuda:0")
        for d in range(3):  # every replica's own tables through the device call
            t_ids = torch.from_numpy(np.asarray(lane_ids[:6], np.uint32).view(np.int32).copy()).to(dev)
            t_sig = torch.from_numpy(np.frombuffer(b"".join(sigs[:6]), np.uint8).reshape(6, 64).copy()).to(dev)
            t_msg = torch.from_numpy(np.frombuffer(b"".join(msgs[:6]), np.uint8).reshape(6, 32).copy()).to(dev)
            t_st = torch.full((6,), 0xA5, dtype=torch.uint8, device=dev)
            eng.ed25519_verify_keyed_device(t_ids, t_sig, t_msg, t_st, None, device=d,
                                            stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
            assert np.array_equal(t_st.cpu().numpy(), got[:6]), d


# ---- 9. three chunks of one call: dense, CSR, a two-lane tail ---------------------------------
@pytest.fixture(scope="module")
def three_chunks(oracle, five):
    """130 lanes for CORDAHIP_HOST_CHUNK=64, signed and judged by the oracle once: chunk 0 all
    32-byte messages (dense rows), chunk 1 mixed lengths with 0- and 33-byte messages (CSR: the
    offset and length buffers are first needed in the middle of the call), chunk 2 a 2-lane tail."""
    ids, seeds, pubs = five
    lens = [32] * 64 + [(0, 33, 32, 1, 31, 64, 100)[i % 7] for i in range(64)] + [32, 32]
    n = len(lens)
    msgs = [hashlib.shake_256(b"vkey-3chunk-%d" % i).digest(lens[i]) for i in range(n)]
    sigs = [bytearray(csign(oracle, seeds[i % 5], msgs[i])[1]) for i in range(n)]
    for i in range(0, n, 6):
        sigs[i][i % 64] ^= 0x04
    sigs[70], sigs[129] = sigs[70][:63], sigs[129] + b"\0"  # not 64 bytes: the host's pre-status
    sigs = [bytes(s) for s in sigs]
    want = np.zeros(n, np.uint8)
    for L in sorted(set(lens)):  # the oracle's batch takes dense rows: one call per length
        sel = [i for i in range(n) if lens[i] == L and len(sigs[i]) == 64]
        want[sel] = oracle_statuses(oracle, [pubs[i % 5] for i in sel], [sigs[i] for i in sel], [msgs[i] for i in sel])
    want[[70, 129]] = MALFORMED_SIG  # EdDSAEngine: signature length (both messages are non-empty)
    assert lens[70] and {OK, BAD_SIG, EMPTY} <= set(want.tolist()) and (want[64:128] == OK).sum() > 32
    return [ids[i % 5] for i in range(n)], sigs, msgs, want


@pytest.mark.parametrize("with_verdict", [True, False])
def test_three_chunks_dense_csr_tail(engine, three_chunks, monkeypatch, with_verdict):
    """The chunk loop's three shapes in one call, with and without verdict words; with them, run()
    checks that the tail's word has no bit set past lane 129."""
    monkeypatch.setenv("CORDAHIP_HOST_CHUNK", "64")
    lane_ids, sigs, msgs, want = three_chunks
    got = HostBatch(lane_ids, sigs, msgs).run(engine, verdict=with_verdict)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), len(msgs[i]), int(got[i]), int(want[i])) for i in bad[:10]]
