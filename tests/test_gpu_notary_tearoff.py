"""Notary tear-offs from typed inputs and time windows on the GPU (K21 + K6, then K16):
cordahip_notary_tearoff_verify / _submit / _device / _commit / _commit_submit and
resolve.notarise_tearoffs against what the library already answers for the same
tear-offs with their leaves serialised (Engine.filtered_tx_verify over the leaves of
tests/kryo_notary_model.py, Engine.commit_inputs' model tests/commit_log_model.py,
resolve.notarise_filtered_transactions). The leaves are PARITY UNPINNED (the model and
the encoder restate the same published Kryo rules)."""
import ctypes
import functools
import hashlib
import random

import numpy as np
import pytest

import kryo_notary_model as M
from commit_log_model import CommitLogModel
from corda_amd import _lib, resolve
from corda_amd._lib import lib

pytestmark = pytest.mark.gpu
OK, BAD_SIG, NO_LEAVES, BAD_TREE, BAD_COMPONENT = 0, 1, 6, 8, 9
REF_COUNTS = [0, 1, 2, 3, 5, 8, 9]  # Merkle widths 1..16, padded and unpadded


def _h(tag) -> bytes:
    return hashlib.sha256(tag if isinstance(tag, bytes) else tag.encode()).digest()


def _window(rng):
    side = lambda: (rng.choice(M.SECOND_EDGES[:5] + [1500000000 + rng.randrange(10**6)]), rng.choice(M.NANO_EDGES))  # noqa: E731
    return rng.choice([(side(), side()), (side(), None), (None, side()), (None, None)])


def _spec(rng, tag, nref, win):
    refs = [(_h("%s ref %d" % (tag, i)), rng.choice(M.INDEX_EDGES + [rng.randrange(2**32)])) for i in range(nref)]
    raws = [bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 40))) for _ in range(rng.randrange(1, 4))]
    return refs, (_window(rng) if win else None), raws


def _typed_leaves(refs, window):
    """availableComponents order of what the typed form names: the refs, then the window."""
    return [M.state_ref_leaf(h, i) for h, i in refs] + ([M.time_window_leaf(*window)] if window is not None else [])


def _build(engine, specs, reveal_raw=()):
    """Tear-offs (refs, window, tokens, root) of transactions whose other leaves are RAW bytes, built
    with Engine.filtered_tx_build revealing exactly refs + window (reveal_raw: also the first RAW
    leaf; a transaction with nothing to reveal shows its first RAW leaf, to have a tree at all)."""
    txs = []
    for t, (refs, window, raws) in enumerate(specs):
        nothing = not refs and window is None
        leaves = [M.state_ref_leaf(h, i) for h, i in refs] + list(raws)
        inc = [True] * len(refs) + [(t in reveal_raw or nothing) and k == 0 for k in range(len(raws))]
        if window is not None:
            leaves.append(M.time_window_leaf(*window))
            inc.append(True)
        txs.append((leaves, inc))
    ids, st, toks = engine.filtered_tx_build(txs)
    assert not st.any()
    return [(list(refs), window, toks[t], ids[t].tobytes()) for t, (refs, window, _) in enumerate(specs)]


@functools.lru_cache(maxsize=None)
def _corpus_specs(n):
    rng = random.Random(2100 + n)
    return [_spec(rng, "c%d" % t, REF_COUNTS[t % 7], (t // 7) % 2 == 0) for t in range(n)]


_CORPUS = {}


def _corpus(engine, n):
    if n not in _CORPUS:
        _CORPUS[n] = _build(engine, _corpus_specs(n))
    return [(list(r), w, k, root) for r, w, k, root in _CORPUS[n]]


def _expected(engine, tearoffs):
    """filtered_tx_verify over the model's serialised leaves; BAD_COMPONENT where the window is no item."""
    bad = [w is not None and not M.window_valid(*w) for _, w, _, _ in tearoffs]
    ftxs = [(_typed_leaves(r, None if b else w), k, root) for (r, w, k, root), b in zip(tearoffs, bad)]
    want = [int(x) for x in engine.filtered_tx_verify(ftxs)]
    return [BAD_COMPONENT if b else x for x, b in zip(want, bad)]


@pytest.mark.parametrize("ntx", [1, 2, 67, 300])
def test_valid_corpus_matches_serialised_verify(engine, ntx):
    tearoffs = _corpus(engine, ntx)
    want = _expected(engine, tearoffs)
    assert want == [NO_LEAVES if (not r and w is None) else OK for r, w, _, _ in tearoffs]
    assert [int(x) for x in engine.notary_tearoff_verify(tearoffs)] == want
    assert [int(x) for x in engine.notary_tearoff_verify(tearoffs, async_=True).wait()] == want


def test_a_transaction_whose_leaves_cross_a_block(engine):
    rng = random.Random(300)
    tearoffs = _build(engine, [_spec(rng, "a", 3, True), _spec(rng, "big", 300, True), _spec(rng, "z", 2, False)])
    st, lh = engine.notary_tearoff_verify(tearoffs, leaf_hash=True)
    assert [int(x) for x in st] == _expected(engine, tearoffs) == [OK, OK, OK]
    want = [M.sha256(leaf) for r, w, _, _ in tearoffs for leaf in _typed_leaves(r, w)]
    assert [x.tobytes() for x in lh] == want


def test_mutants_match_serialised_verify(engine):
    tearoffs = _corpus(engine, 67)
    base = _expected(engine, tearoffs)
    by = lambda nref, win: next(t for t in range(14, 67) if len(tearoffs[t][0]) == nref  # noqa: E731
                                and (tearoffs[t][1] is not None) == win and t not in used)
    used, why = set(), {}

    def mutate(name, nref, win, fn, expect):
        t = by(nref, win)
        used.add(t)
        r, w, k, root = tearoffs[t]
        tearoffs[t] = fn(list(r), w) + (k, root)
        why[t] = (name, expect)

    mutate("index changed", 3, True, lambda r, w: ([(r[0][0], r[0][1] ^ 1)] + r[1:], w), BAD_SIG)
    mutate("hash bit flipped", 5, False, lambda r, w: (r[:2] + [(bytes([r[2][0][0] ^ 0x10]) + r[2][0][1:], r[2][1])] + r[3:], w), BAD_SIG)
    mutate("ref dropped", 8, True, lambda r, w: (r[:-1], w), BAD_SIG)
    mutate("ref doubled", 2, False, lambda r, w: (r + r[:1], w), BAD_SIG)
    mutate("refs permuted", 9, True, lambda r, w: (r[::-1], w), OK)
    mutate("refs rotated", 5, True, lambda r, w: (r[2:] + r[:2], w), OK)
    mutate("side toggled", 1, True, lambda r, w: (r, ((5, 0) if w[0] is None else None, w[1])), BAD_SIG)

    def nano_moved(w):  # nanos + 1 (- 1 at the top) on a side that is present; two absent sides get one
        for i in (1, 0):
            if w[i] is not None:
                s, n = w[i]
                moved = (s, n + 1 if n < 999999999 else n - 1)
                return (w[0], moved) if i else (moved, w[1])
        return ((0, 1), None)

    mutate("nano moved", 2, True, lambda r, w: (r, nano_moved(w)), BAD_SIG)
    mutate("window supplied", 3, False, lambda r, w: (r, ((5, 0), None)), BAD_SIG)
    mutate("window withheld", 9, True, lambda r, w: (r, None), BAD_SIG)
    mutate("invalid window row", 8, True, lambda r, w: (r, ((0, 1000000000), None)), BAD_COMPONENT)
    want = _expected(engine, tearoffs)
    for t, (name, expect) in why.items():
        assert want[t] == expect, (name, want[t])
    assert [want[t] for t in range(67) if t not in why] == [base[t] for t in range(67) if t not in why]
    got = [int(x) for x in engine.notary_tearoff_verify(tearoffs)]
    assert got == want, [(why.get(t), got[t], want[t]) for t in range(67) if got[t] != want[t]]


def test_a_revealed_raw_leaf_and_nothing_revealed(engine):
    rng = random.Random(44)
    specs = [_spec(rng, "r0", 2, True), _spec(rng, "r1", 3, False), _spec(rng, "r2", 0, False), _spec(rng, "r3", 1, True)]
    tearoffs = _build(engine, specs, reveal_raw={1})
    want = _expected(engine, tearoffs)
    assert want == [OK, BAD_SIG, NO_LEAVES, OK]  # the typed form cannot name the RAW leaf; no leaves at all
    assert [int(x) for x in engine.notary_tearoff_verify(tearoffs)] == want


def _edge_tearoffs():
    """Every edge ref in transaction 0, one edge window per transaction; no trees (the leaf hashes
    and the windows do not depend on them)."""
    ws = M.edge_windows()
    return [(M.edge_refs() if t == 0 else [], w, [], bytes(32)) for t, w in enumerate(ws)]


def test_leaf_hashes_at_every_edge(engine):
    tearoffs = _edge_tearoffs()
    st, lh = engine.notary_tearoff_verify(tearoffs, leaf_hash=True)
    want = [M.sha256(leaf) for r, w, _, _ in tearoffs for leaf in _typed_leaves(r, w)]
    assert len(lh) == len(want) == len(M.INDEX_EDGES) + len(tearoffs)
    assert [x.tobytes() for x in lh] == want
    assert all(int(x) == BAD_TREE for x in st)  # an empty token stream is no tree


SAT = 4611686018  # 2^62 ns = 4611686018 s + 427387904 ns


def test_device_form_windows_and_hashes(engine):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    windows = [None, (None, None), ((0, 0), None), (None, (0, 1)), ((1500000000, 5), (1500000030, 0)),
               ((M.INSTANT_MAX_SECOND, 999999999), (M.INSTANT_MIN_SECOND, 0)),
               ((SAT, 427387903), (SAT, 427387904)), ((SAT, 427387905), (SAT + 1, 0)),
               ((-SAT - 1, 572612097), (-SAT - 1, 572612096)), ((-SAT - 1, 572612095), (-SAT - 2, 999999999)),
               ((-1, 999999999), (2**34, 128)), ((0, -1), (7, 7)), ((1, 1), (M.INSTANT_MAX_SECOND + 1, 0))]
    tearoffs = [([(_h("d%d" % t), t)], w, [], bytes(32)) for t, w in enumerate(windows)]
    b, keep, off, st, _ = engine._tearoff_arrays(tearoffs, False)
    refs, off_, ko, fl, fs, fn, us, un, tok, th, root = keep[:11]
    n = len(tearoffs)
    up = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if dt is None else a.astype(dt)).to(dev)  # noqa: E731
    d = dict(refs=up(refs).reshape(-1, 36)[:n], tx_ref_off=up(off_, np.int64), tok=torch.zeros(0, dtype=torch.uint8, device=dev),
             tok_hash=torch.zeros((0, 32), dtype=torch.uint8, device=dev), tx_tok_off=up(ko, np.int64),
             root=up(root).reshape(-1, 32))
    status = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    twf = torch.zeros(n, dtype=torch.int64, device=dev)
    twu = torch.zeros(n, dtype=torch.int64, device=dev)
    nleaves = n + sum(w is not None for w in windows)
    lh = torch.zeros((nleaves, 32), dtype=torch.uint8, device=dev)
    engine.notary_tearoff_device(d["refs"], d["tx_ref_off"], d["tok"], d["tok_hash"], d["tx_tok_off"], d["root"], status,
                                 twf, twu, tw_flags=up(fl, np.uint8), tw_from_s=up(fs, np.int64),
                                 tw_from_nano=up(fn, np.int32), tw_until_s=up(us, np.int64),
                                 tw_until_nano=up(un, np.int32), leaf_hash=lh)
    torch.cuda.synchronize(dev)
    valid = [w is None or M.window_valid(*w) for w in windows]
    want_f = [M.instant_ns(w[0]) if w is not None and v else M.ABSENT for w, v in zip(windows, valid)]
    want_u = [M.instant_ns(w[1]) if w is not None and v else M.ABSENT for w, v in zip(windows, valid)]
    assert twf.cpu().tolist() == want_f and twu.cpu().tolist() == want_u
    assert 2**62 in want_f and -2**62 in want_f and 2**62 - 1 in want_f and -2**62 + 1 in want_f
    assert status.cpu().tolist() == [BAD_TREE if v else BAD_COMPONENT for v in valid]
    want_h = []
    for (r, w, _, _), v in zip(tearoffs, valid):
        want_h += [M.sha256(M.state_ref_leaf(*r[0]))]
        if w is not None:
            want_h += [M.sha256(M.time_window_leaf(*w)) if v else bytes(32)]
    assert [bytes(x) for x in lh.cpu().numpy()] == want_h


def test_device_encoder_writes_both_kinds(engine):
    """cordahip_kryo_encode_device of both kinds against the host encoder: twice in one context (the
    second call writes from the templates the first built), and a batch of one item of each kind.
    (The device encoder has no size threshold: the direct path takes items without a shape, which
    for these kinds are only the rows the encoder rejects.)"""
    items = [("state_ref", _lib.pack_state_ref(h, i), 0) for h, i in M.edge_refs()]
    items += [("time_window", _lib.pack_time_window(f, u), 0) for f, u in M.edge_windows()]
    items += [("time_window", _lib.pack_time_window((0, 1000000000), None), 0), ("state_ref", bytes(35), 0)]
    host = _lib.kryo_encode(items[:-2])
    blob, arr, has = _lib.kryo_pack(items)
    for _ in range(2):
        out, off, status = engine.kryo_encode_packed_device(blob, arr, has)
        o = off.cpu().numpy()
        leaves = out.cpu().numpy()
        assert status.cpu().tolist() == [0] * len(host) + [1, 1]
        assert [leaves[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(host))] == host
    for i in (0, len(M.INDEX_EDGES)):
        blob1, arr1, has1 = _lib.kryo_pack(items[i:i + 1])
        out, off, status = engine.kryo_encode_packed_device(blob1, arr1, has1)
        assert status.cpu().tolist() == [0] and out.cpu().numpy().tobytes() == host[i]


def _ns_window(w):
    if w is None:
        return None
    f, u = M.instant_ns(w[0]), M.instant_ns(w[1])
    return (None if f == M.ABSENT else f, None if u == M.ABSENT else u)


NOW = 1500000010 * 10**9
TOL = 30 * 10**9


def _commit_corpus(engine):
    rng = random.Random(77)
    specs = [_spec(rng, "k%d" % t, REF_COUNTS[1 + t % 6], False) for t in range(40)]
    win = lambda f, u: ((1500000000 + f, 5), (1500000000 + u, 0))  # noqa: E731
    for t in range(0, 40, 3):
        specs[t] = (specs[t][0], win(0, 30), specs[t][2])
    specs[4] = (specs[4][0], win(-100, -50), specs[4][2])        # closed 50 s ago: invalid beyond the tolerance
    specs[5] = (specs[5][0], (None, (1500000000 - 41, 0)), specs[5][2])
    specs[7] = (specs[7][0], ((1500000000 + 41, 0), None), specs[7][2])   # opens in 31 s
    specs[9] = (specs[9][0][:1] + specs[2][0][:1], None, specs[9][2])     # spends a ref of transaction 2: conflict
    specs[11] = specs[3]                                                   # transaction 3 again: already committed
    return _build(engine, specs)


def _check_commit(engine, log_id, model, tearoffs, callers, gate=None, run=None):
    vexp = _expected(engine, tearoffs)
    txs = [(root, c, r, _ns_window(w) if v != BAD_COMPONENT else None) for (r, w, _, root), c, v in zip(tearoffs, callers, vexp)]
    mgate = [int(v != OK or (gate is not None and gate[t])) for t, v in enumerate(vexp)]
    mst, mcm, mrs, mrb = model.commit_batch(txs, NOW, TOL, mgate)
    want = [v if v != OK else s for v, s in zip(vexp, mst)]
    st, cm, rs, rb = run() if run else engine.notary_tearoff_commit(log_id, tearoffs, callers, NOW, TOL, gate=gate)
    assert [int(x) for x in st] == want
    assert [int(x) for x in cm] == mcm and rs == mrs and rb == mrb
    return want, mcm


def test_commit_against_the_model(engine):
    log_id = engine.commit_log_create(12)
    try:
        model = CommitLogModel()
        tearoffs = _commit_corpus(engine)
        callers = [7 + t % 3 for t in range(40)]
        callers[11] = callers[3]
        gate = [0] * 40
        gate[13] = gate[14] = 1
        # one tear-off's ref rows altered after the build: not proven, so not committed
        r, w, k, root = tearoffs[20]
        original = list(r)
        tearoffs[20] = ([(r[0][0], r[0][1] ^ 1)] + r[1:], w, k, root)
        want, cm = _check_commit(engine, log_id, model, tearoffs, callers, gate)
        assert want[20] == BAD_SIG and cm[20] == 0
        assert engine.commit_log_lookup(log_id, tearoffs[20][0] + original) == [None] * (2 * len(original))
        assert want[4] == want[5] == want[7] == 17 and want[9] == 16 and want[13] == want[14] == 18
        assert want[11] == OK and cm[11] == 0 and cm[3] == 1 and cm[0] == 1
        # the whole batch again, by the same callers: everything that committed is already committed
        want2, cm2 = _check_commit(engine, log_id, model, tearoffs, callers, gate)
        assert not any(cm2) and [w for w in want2 if w == OK]
        entries, _, _ = engine.commit_log_stats(log_id)
        assert entries == len(model.log)
    finally:
        engine.commit_log_destroy(log_id)


def test_two_tickets_commit_in_order(engine):
    log_id = engine.commit_log_create(10)
    try:
        rng = random.Random(5)
        a = _build(engine, [_spec(rng, "t%d" % t, 2, t % 2 == 0) for t in range(6)])
        b = [a[2], a[5]] + _build(engine, [(a[1][0][:1] + _spec(rng, "u", 1, False)[0], None, [b"x"])])
        ta = engine.notary_tearoff_commit(log_id, a, [1] * 6, NOW, 10**18, async_=True)
        tb = engine.notary_tearoff_commit(log_id, b, [1, 2, 1], NOW, 10**18, async_=True)
        sb, cb, _, rbb = tb.wait()
        sa, ca, _, _ = ta.wait()
        assert [int(x) for x in sa] == [OK] * 6 and [int(x) for x in ca] == [1] * 6
        # the second ticket saw the first's commits: same tx and caller again, same tx by another caller, a spent ref
        assert [int(x) for x in sb] == [OK, 16, 16] and [int(x) for x in cb] == [0, 0, 0]
        assert rbb[2][0] == (a[1][3], 0, 1) and rbb[2][1] is None
    finally:
        engine.commit_log_destroy(log_id)


def test_notarise_tearoffs_equals_notarise_filtered_transactions(engine):
    key_id, _ = engine.signer_add_ed25519(_h("notary key"))
    logs = [engine.commit_log_create(12), engine.commit_log_create(12)]
    try:
        tearoffs = _commit_corpus(engine)
        r, w, k, root = tearoffs[20]
        tearoffs[20] = ([(r[0][0], r[0][1] ^ 1)] + r[1:], w, k, root)
        callers = [7 + t % 3 for t in range(40)]
        callers[11] = callers[3]
        ftxs = [(_typed_leaves(r, w), k, root) for r, w, k, root in tearoffs]
        inputs = [r for r, _, _, _ in tearoffs]
        windows = [_ns_window(w) for _, w, _, _ in tearoffs]
        for _ in range(2):  # the second round: everything already committed, signed again
            want = resolve.notarise_filtered_transactions(engine, logs[0], ftxs, inputs, windows, callers, key_id, NOW, TOL)
            got = resolve.notarise_tearoffs(engine, logs[1], tearoffs, callers, key_id, NOW, TOL)
            assert got == want
        kinds = {type(a).__name__ if isinstance(a, bytes) else a.kind for a in want[0]}
        assert kinds == {"bytes", "TransactionInvalid", "TimeWindowInvalid", "Conflict"}
        seen = []
        got = resolve.notarise_tearoffs_persisted(engine, logs[1], tearoffs[:3], callers[:3], key_id, NOW, TOL, seen.append)
        assert seen == [got[1]]
    finally:
        for log_id in logs:
            engine.commit_log_destroy(log_id)
        engine.signer_remove(key_id)


@pytest.mark.parametrize("entry", ["verify", "submit", "commit", "commit_submit"])
@pytest.mark.parametrize("which", ["ref_order", "ref_end", "tok_end", "window_pairing"])
def test_bad_offsets_are_invalid_arg_and_touch_nothing(engine, entry, which):
    tearoffs = _corpus(engine, 67)[:20]
    n = len(tearoffs)
    b, keep, off, st, _ = engine._tearoff_arrays(tearoffs, False)
    ko = keep[2]
    if which == "ref_order":
        off[5] = off[6] + 1
    elif which == "ref_end":
        off[n] += 1
    elif which == "tok_end":
        ko[n] += 1
    else:
        b.tw_until_nano = None
    st[:] = 0xAA
    caller = np.ones(n, np.uint32)
    cm = np.full(n, 0xAA, np.uint8)
    rs = np.full(int(b.n_refs) + 1, 0xAA, np.uint8)
    rb = np.zeros(int(b.n_refs) + 1, _lib.CONSUMING_TX_DTYPE)
    log_id = engine.commit_log_create(10)
    try:
        before = engine.commit_log_stats(log_id)
        ticket = ctypes.c_uint64()
        cargs = (engine.ctx, log_id, ctypes.byref(b), caller.ctypes.data, NOW, TOL, None, cm.ctypes.data, rs.ctypes.data,
                 rb.ctypes.data)
        if entry == "verify":
            rc = lib().cordahip_notary_tearoff_verify(engine.ctx, ctypes.byref(b))
        elif entry == "commit":
            rc = lib().cordahip_notary_tearoff_commit(*cargs)
        else:
            rc = (lib().cordahip_notary_tearoff_submit(engine.ctx, ctypes.byref(b), ctypes.byref(ticket)) if entry == "submit"
                  else lib().cordahip_notary_tearoff_commit_submit(*cargs, ctypes.byref(ticket)))
            assert rc == 0
            rc = lib().cordahip_wait(engine.ctx, ticket.value, -1)
        assert rc == _lib.ERR_INVALID_ARG
        assert (st == 0xAA).all() and (cm == 0xAA).all() and (rs == 0xAA).all()
        assert engine.commit_log_stats(log_id) == before and before[0] == 0
    finally:
        engine.commit_log_destroy(log_id)
