"""cordahip_txcomp_inputs_device (K22) against the model of its rule
(tests/kryo_payment_model.py extract_inputs): a component batch's STATE_REF items as commit
rows, its TIME_WINDOW items as window bounds, and the gate. ntx 1025 gives the one-block scan
more than one transaction per thread. Every comparison is exact."""
import functools
import random

import numpy as np
import pytest

import kryo_notary_model as N
import kryo_payment_model as M
from corda_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 0xEE
WINDOWS = [
    ((1500000000, 5), (1500000030, 0)), ((1500000000, 5), None), (None, (1500000030, 999999999)), (None, None),
    ((4611686018, 427387904), (N.INSTANT_MAX_SECOND, 0)),  # saturating at +2^62
    ((N.INSTANT_MIN_SECOND, 0), (-4611686019, 572612095)),  # saturating at -2^62
    ((-1, 0), (0, 0)),
]


@functools.lru_cache(maxsize=None)
def _batch(ntx):
    """(items [(kind, offset, len)], payload bytes, tx_item_off list) with, when ntx allows, every
    case of the issue at a fixed transaction."""
    rng = random.Random(900 + ntx)
    payload, items, tio = bytearray(b"\x07" * rng.randrange(1, 4)), [], [0]  # rows at odd byte offsets

    def put(kind, b, length=None):
        items.append((kind, len(payload), len(b) if length is None else length))
        payload.extend(b)

    def ref():
        put(16, bytes(rng.randrange(256) for _ in range(32)) + rng.choice(N.INDEX_EDGES).to_bytes(4, "little"))

    def other():
        put(rng.choice([0, 10, 12, 13, 14, 15, 18, 19, 99]), bytes(rng.randrange(256) for _ in range(rng.randrange(0, 50))))

    late = {}  # transaction -> what to patch once the payload is complete
    for t in range(ntx):
        case = t % 67 if ntx >= 67 else -1
        if t % 5 == 3:  # an issue between payments: no refs
            for _ in range(rng.randrange(1, 6)):
                other()
        else:
            for _ in range(rng.randrange(1, 4)):
                ref()
            for _ in range(rng.randrange(2, 6)):
                other()
            if case == 10:
                put(16, bytes(36), 35)  # a STATE_REF of length 35
            if case == 11:
                put(16, bytes(36), 37)
            if case == 12:
                ref()
                late[len(items) - 1] = "short"  # its offset becomes payload_len - 35
            if case == 14:
                put(16, bytes(36))
                late[len(items) - 1] = "far"
            w = rng.randrange(len(WINDOWS) + 2)
            if w < len(WINDOWS):
                put(17, _lib.pack_time_window(*WINDOWS[w]))
            if case == 20:  # duplicated
                put(17, _lib.pack_time_window(*WINDOWS[0]))
                put(17, _lib.pack_time_window(*WINDOWS[0]))
            if case == 21:  # invalid rows: flags, a nano out of range, a wrong length, out of the payload
                put(17, b"\x04" + bytes(24))
            if case == 22:
                put(17, b"\x01" + bytes(8) + (1000000000).to_bytes(4, "little") + bytes(12))
            if case == 25:
                put(17, _lib.pack_time_window(*WINDOWS[0]), 24)
            if case == 24:
                put(17, _lib.pack_time_window(*WINDOWS[0]))
                late[len(items) - 1] = "far"
        tio.append(len(items))
    for i, what in late.items():
        k, _, ln = items[i]
        items[i] = (k, len(payload) - 35 if what == "short" else len(payload) + 2**33, ln)
    if ntx >= 67:  # offsets beyond n_items, one in the middle (two ranges change) and the last
        tio[40] = 2**40
        tio[ntx] = len(items) + 5
    return items, bytes(payload), tio


def _call(engine, items, payload, tio, ref_cap, status):
    import torch
    dev = torch.device("cuda:0")
    ntx = len(tio) - 1
    arr = np.zeros(len(items), _lib.KRYO_ITEM_DTYPE)
    arr["kind"], arr["data"], arr["len"] = [k for k, _, _ in items], [o for _, o, _ in items], [n for _, _, n in items]
    d_items = torch.from_numpy(arr.view(np.uint8).copy()).to(dev) if len(items) else torch.zeros(32, dtype=torch.uint8, device=dev)
    d_payload = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(dev)
    d_tio = torch.from_numpy(np.asarray(tio, np.uint64).view(np.int64).copy()).to(dev)
    refs = torch.full((ref_cap + 3, 36), GUARD, dtype=torch.uint8, device=dev)
    tro = torch.full((ntx + 1,), -7, dtype=torch.int64, device=dev)
    tw_from, tw_until = torch.full((ntx,), 7, dtype=torch.int64, device=dev), torch.full((ntx,), 7, dtype=torch.int64, device=dev)
    gate = torch.full((ntx,), 0x55, dtype=torch.uint8, device=dev)
    d_status = torch.from_numpy(np.asarray(status, np.uint8)).to(dev) if status is not None else None
    engine.txcomp_inputs_device(d_items, len(items), d_payload, d_tio, refs, tro, tw_from, tw_until, gate,
                                tx_status=d_status, ref_cap=ref_cap)
    torch.cuda.synchronize()
    return refs.cpu().numpy(), tro.cpu().numpy(), tw_from.cpu().numpy(), tw_until.cpu().numpy(), gate.cpu().numpy()


@pytest.mark.parametrize("ntx", [1, 2, 67, 300, 1025])
def test_inputs_windows_and_gate_equal_the_model(engine, ntx):
    items, payload, tio = _batch(ntx)
    total = M.extract_inputs(items, payload, tio, 2**62)[1][ntx]
    assert total > 0
    rng = random.Random(ntx)
    given = [rng.choice([0, 0, 0, 1, 7, 9, 10]) for _ in range(ntx)]
    seen = set()
    for ref_cap in (total, total - 1, 0):
        for status in (None, given):
            rows, off, f, u, gate = M.extract_inputs(items, payload, tio, ref_cap, status)
            got_refs, got_off, got_f, got_u, got_gate = _call(engine, items, payload, tio, ref_cap, status)
            ctx = (ntx, ref_cap, status is not None)
            assert got_off.tolist() == off, ctx
            assert got_f.tolist() == f and got_u.tolist() == u, ctx
            assert got_gate.tolist() == gate, ctx
            assert got_refs[:len(rows)].tobytes() == b"".join(rows), ctx
            assert (got_refs[len(rows):] == GUARD).all(), ctx  # below ref_cap and the guard rows after it
            seen |= set(gate)
    assert M.TX_BAD_COMPONENT in seen and 0 in seen
    if ntx >= 67:
        rows, off, f, u, gate = M.extract_inputs(items, payload, tio, total)
        for t in (10, 11, 12, 14, 20, 21, 22, 24, 25):  # each case flags its transaction, whose range is empty
            assert t % 5 != 3 and gate[t] == M.TX_BAD_COMPONENT and off[t] == off[t + 1], t
            assert f[t] == u[t] == N.ABSENT
        assert 2**62 in f + u and -2**62 in f + u  # the saturating windows came through
        assert any(a == N.ABSENT and b != N.ABSENT for a, b in zip(f, u))  # one-sided


def test_invalid_arguments_touch_nothing(engine):
    import torch
    dev = torch.device("cuda:0")
    items, payload, tio = _batch(2)
    arr = np.zeros(len(items), _lib.KRYO_ITEM_DTYPE)
    arr["kind"], arr["data"], arr["len"] = [k for k, _, _ in items], [o for _, o, _ in items], [n for _, _, n in items]
    d_items = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
    d_payload = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(dev)
    d_tio = torch.from_numpy(np.asarray(tio, np.int64)).to(dev)
    outs = [torch.full((8, 36), GUARD, dtype=torch.uint8, device=dev), torch.full((3,), -7, dtype=torch.int64, device=dev),
            torch.full((2,), 7, dtype=torch.int64, device=dev), torch.full((2,), 7, dtype=torch.int64, device=dev),
            torch.full((2,), 0x55, dtype=torch.uint8, device=dev)]
    before = [o.cpu().numpy().copy() for o in outs]
    f = _lib.lib().cordahip_txcomp_inputs_device
    p = [o.data_ptr() for o in outs]

    def call(ctx=engine.ctx, device=0, n_items=len(items), ntx=2, refs=p[0], off=p[1], fr=p[2], un=p[3], gate=p[4]):
        return f(ctx, device, d_items.data_ptr(), n_items, d_payload.data_ptr(), len(payload), d_tio.data_ptr(), ntx,
                 None, refs, 8, off, fr, un, gate, 0)

    assert call(ctx=None) == _lib.ERR_INVALID_ARG
    assert call(device=99) == _lib.ERR_INVALID_ARG and call(device=-1) == _lib.ERR_INVALID_ARG
    for k in ("refs", "off", "fr", "un", "gate"):
        assert call(**{k: None}) == _lib.ERR_INVALID_ARG, k
    assert call(n_items=2**31 - 1) == _lib.ERR_INVALID_ARG
    assert call(off=p[1] + 4) == _lib.ERR_INVALID_ARG  # a misaligned 64-bit array
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert np.array_equal(o.cpu().numpy(), b)
    assert call(ntx=0) == 0  # a successful no-op
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert np.array_equal(o.cpu().numpy(), b)
    assert call() == 0
    torch.cuda.synchronize()
    assert outs[1].cpu().numpy().tolist() == M.extract_inputs(items, payload, tio, 8)[1]
