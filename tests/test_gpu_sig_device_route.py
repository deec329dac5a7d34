"""Registered-key routing inside the mixed device-resident calls (K24:
cordahip_vkey_set_routing_device). The reference of every case is the same call with the device
switch off: statuses and verdict words must be equal lane for lane, and each family's route
counters must move by what a host replay of the rule gives for the rows the packer sends to that
family's verifier (sig_pack.hpp lane_rule; the match rules of K14, K15 and K20)."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bc_ecdsa as ec
import bc_rsa_pss as bc
from corda_amd import _lib
from test_gpu_rsa_route import by_class, load_keys, pooled
from test_gpu_sig_device import (BAD_RANGE, Dev, _comp_corpora, _dev_comp, _dev_sig_args, _mixed_sigs, _results,
                                 mix, model_status, rsa_rows, run_rows)  # noqa: F401 (mix: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSA, ED = 1, 4
ALL = (True, True, True)


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own: its registry and its counters"""
    from corda_amd.engine import Engine
    with Engine(1) as e:
        yield e


class Reg:
    """the test's own books of the live keys: what the rule may match"""

    def __init__(self):
        self.ed, self.ec, self.rsa, self.ids = set(), set(), set(), {}

    def add_ed(self, e, key):
        kid, st = e.vkey_add_ed25519(key)
        assert st == _lib.OK and any(key)
        self.ed.add(key)
        self.ids[(ED, key)] = kid
        return kid

    def add_ec(self, e, sch, pk):
        assert len(pk) == 65
        kid, st = e.vkey_add_ecdsa(sch, pk)[:2]
        assert st == _lib.OK
        self.ec |= {(sch, pk), (sch, ec.compress(pk))}
        self.ids[(sch, pk)] = kid
        return kid

    def add_rsa(self, e, k):
        kid, st = e.vkey_add_rsa(k["der"])[:2]
        assert st == _lib.OK
        self.rsa.add((k["n"], k["e"]))
        self.ids[(RSA, k["der"])] = kid
        return kid

    def has(self, row):
        sch, k = row[0], row[1]
        if sch == ED:
            return k in self.ed
        if sch in (2, 3):
            return (sch, k) in self.ec
        kk = bc.decode_key(k) if sch == RSA else 0
        return not isinstance(kk, int) and kk in self.rsa


def rule_counts(rows, reg, is_valid=False, rsa=True, fam=ALL):
    """(keyed, generic) per family, of the rows the packer sends to that family's verifier; a family
    whose switch is off or that has no live key routes nothing"""
    out = [[0, 0], [0, 0], [0, 0]]
    for row in rows:
        sch, k, s, m = row
        if sch in (2, 3):
            if len(k) not in (33, 65):
                continue
            f = 1
        elif sch == RSA:
            kk = bc.decode_key(k) if rsa else 0
            if isinstance(kk, int) or (not is_valid and (len(s) == 0 or len(m) == 0)):
                continue
            if len(s) > (kk[0].bit_length() + 7) // 8:
                continue
            f = 2
        elif sch == ED and len(k) == 32:
            f = 0
        else:
            continue
        out[f][0 if reg.has(row) else 1] += 1
    live = (bool(reg.ed), bool(reg.ec), bool(reg.rsa))
    return tuple(tuple(c) if on and lv else (0, 0) for c, on, lv in zip(out, fam, live))


def switches(e, fam, dev):
    e.vkey_set_routing(fam[0])
    e.vkey_set_routing_ecdsa(fam[1])
    e.vkey_set_routing_rsa(fam[2])
    e.vkey_set_routing_device(dev)


def stats(e):
    return e.vkey_route_stats(), e.vkey_route_stats_ecdsa(), e.vkey_route_stats_rsa()


def moved(before, after):
    return tuple((a[0] - b[0], a[1] - b[1]) for b, a in zip(before, after))


def both(e, reg, rows, msg_len, is_valid=False, fam=ALL, rsa=True):
    """the batch with the device switch off (the reference) and on: equal results, counters by the rule"""
    try:
        switches(e, fam, False)
        b0 = stats(e)
        off = run_rows(e, rows, msg_len, is_valid=is_valid, rsa=rsa)
        assert stats(e) == b0  # device switch off, family switches on: no counter moves
        switches(e, fam, True)
        on = run_rows(e, rows, msg_len, is_valid=is_valid, rsa=rsa)
        mv = moved(b0, stats(e))
    finally:
        switches(e, (False, False, False), False)
    bad = [(i, rows[i][0], on[0][i], off[0][i]) for i in range(len(rows)) if on[0][i] != off[0][i]]
    assert not bad, bad[:10]
    assert on[1] == off[1] == [int(g == 0) for g in off[0]]
    assert mv == rule_counts(rows, reg, is_valid, rsa, fam), (mv, rule_counts(rows, reg, is_valid, rsa, fam))
    return off[0], mv


@pytest.fixture(scope="module")
def reg(eng, mix):
    """some of the mix's Ed25519, secp256k1, P-256 and RSA keys registered; in each family the keys
    of the 32-byte-message lanes come first, so that the tests over those lanes meet keyed rows"""
    rows, groups = mix
    r = Reg()
    first = [rows[i] for i in groups[32]]
    ed_keys = list(dict.fromkeys(x[1] for x in first + rows if x[0] == ED and len(x[1]) == 32))
    for k in ed_keys[:24:2]:
        r.add_ed(eng, k)
    for sch in (2, 3):
        pks = list(dict.fromkeys(x[1] for x in first + rows if x[0] == sch and len(x[1]) == 65))
        for pk in pks[:10:2]:
            r.add_ec(eng, sch, pk)
    keys = load_keys()
    r.add_rsa(eng, by_class(keys, 64)[0])
    r.add_rsa(eng, by_class(keys, 96)[0])
    return r


# ---- 1. the adversarial mix against the unrouted call ---------------------------------------------
@pytest.mark.parametrize("is_valid", [False, True])
def test_mix_routed_equals_unrouted_and_counters_follow_the_rule(eng, oracle, mix, reg, is_valid):
    rows, groups = mix
    total = [[0, 0], [0, 0], [0, 0]]
    want = model_status(oracle, rows, is_valid)
    for ln, idx in sorted(groups.items()):
        sub = [rows[i] for i in idx]
        got, mv = both(eng, reg, sub, ln, is_valid=is_valid)
        assert got == [want[i] for i in idx], ln
        for f in range(3):
            total[f][0] += mv[f][0]
            total[f][1] += mv[f][1]
    # every family had keyed and generic rows
    assert all(k >= 10 and g >= 10 for k, g in total), total


def test_switch_combinations(eng, mix, reg):
    rows, groups = mix
    sub = [rows[i] for i in groups[32]]
    full = rule_counts(sub, reg)
    assert all(k and g for k, g in full), full
    for off_family in range(3):
        fam = tuple(f != off_family for f in range(3))
        _, mv = both(eng, reg, sub, 32, fam=fam)
        assert mv[off_family] == (0, 0) and all(mv[f] == full[f] for f in range(3) if f != off_family)
    # the device switch alone routes nothing
    _, mv = both(eng, reg, sub, 32, fam=(False, False, False))
    assert mv == ((0, 0),) * 3
    # without the RSA flag no RSA row exists: its counters stay
    _, mv = both(eng, reg, sub, 32, rsa=False)
    assert mv[2] == (0, 0) and mv[0] == full[0] and mv[1] == full[1]


# ---- 2. batch sizes and classes ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_batches_all_none_and_one_keyed(eng, mix, reg, n):
    rows, groups = mix
    sub = [rows[i] for i in groups[32]]
    taken = [r for r in sub if sum(map(sum, rule_counts([r], reg))) == 1]  # rows some verifier takes
    keyed = [r for r in taken if reg.has(r)]
    plain = [r for r in taken if not reg.has(r)]
    assert len(keyed) >= 65 and len(plain) >= 65 and {r[0] for r in keyed} == {RSA, 2, 3, ED}
    _, mv = both(eng, reg, keyed[:n], 32)
    assert sum(k for k, _ in mv) == n and sum(g for _, g in mv) == 0
    _, mv = both(eng, reg, plain[:n], 32)
    assert sum(k for k, _ in mv) == 0 and sum(g for _, g in mv) == n
    if n:
        for one in keyed[:4] + [r for r in keyed if r[0] == RSA][:1]:
            lanes = list(plain[:n])
            lanes[37 % n] = one
            _, mv = both(eng, reg, lanes, 32)
            assert sum(k for k, _ in mv) == 1 and sum(g for _, g in mv) == n - 1


def test_family_absent_and_each_class_alone(eng, mix, reg):
    rows, groups = mix
    sub = [rows[i] for i in groups[32]]
    picks = {
        "ed25519": [r for r in sub if r[0] == ED and len(r[1]) == 32],
        "ecdsa": [r for r in sub if r[0] in (2, 3) and len(r[1]) in (33, 65)],
        "k1": [r for r in sub if r[0] == 2 and len(r[1]) in (33, 65)],
        "r1": [r for r in sub if r[0] == 3 and len(r[1]) in (33, 65)],
        "no rsa": [r for r in sub if r[0] != RSA],
        "direct": [r for r in sub if r[0] not in (RSA, 2, 3, ED)],
    }
    keys = load_keys()
    for w in (64, 96, 128):
        ders = {k["der"] for k in by_class(keys, w)}
        picks["rsa%d" % w] = [r for r in sub if r[0] == RSA and r[1] in ders]
    for name, lanes in picks.items():
        lanes = lanes[:130]
        assert len(lanes) >= 10, name
        _, mv = both(eng, reg, lanes, 32)
        # a batch with no row of a family leaves that family's counters alone, live key or not
        if name == "ed25519":
            assert mv[0][0] and mv[0][1] and mv[1] == mv[2] == (0, 0)
        elif name in ("ecdsa", "k1", "r1"):
            assert mv[1][0] and mv[1][1] and mv[0] == mv[2] == (0, 0)
        elif name == "no rsa":
            assert mv[0][0] and mv[1][0] and mv[2] == (0, 0)
        elif name == "direct":
            assert mv == ((0, 0),) * 3
        else:
            assert mv[0] == mv[1] == (0, 0) and sum(mv[2]) > 0
            assert (mv[2][0] > 0) == (name in ("rsa64", "rsa96")) and (mv[2][1] > 0 or name != "rsa128")


# ---- 3. tile and launch boundaries ------------------------------------------------------------------
def _repeat(lanes, n):
    assert lanes
    return [lanes[i % len(lanes)] for i in range(n)]


def test_ed25519_rows_past_a_route_tile(eng, mix, reg):
    rows, groups = mix
    lanes = [rows[i] for i in groups[32] if rows[i][0] == ED and len(rows[i][1]) == 32]
    _, mv = both(eng, reg, _repeat(lanes, 2049), 32)
    assert sum(mv[0]) == 2049 and mv[0][0] > 200 and mv[0][1] > 200


def test_ecdsa_rows_past_a_route_tile(eng, mix, reg):
    rows, groups = mix
    lanes = [rows[i] for i in groups[32] if rows[i][0] in (2, 3) and len(rows[i][1]) in (33, 65)]
    assert {(r[0], len(r[1])) for r in lanes} == {(2, 33), (2, 65), (3, 33), (3, 65)}
    assert {(r[0], len(r[1])) for r in lanes if reg.has(r)} == {(2, 33), (2, 65), (3, 33), (3, 65)}
    _, mv = both(eng, reg, _repeat(lanes, 4097), 32)
    assert sum(mv[1]) == 4097 and mv[1][0] > 200 and mv[1][1] > 200


def launch_loop_results(e):
    """130 RSA-2048 rows, every other one on a registered key, some with a flipped bit; the device
    switch off and on. 64-row workspace: three launches (64, 64, 2), each with its own clipped count."""
    keys = by_class(load_keys(), 64)
    reg = Reg()
    reg.add_rsa(e, keys[0])
    rows = []
    for i in range(130):
        k = keys[0] if i % 2 == 0 or i in (63, 65, 127, 129) else keys[1 + i % (len(keys) - 1)]
        m, sig = pooled(k, i, flip=i % 5 == 4)
        rows.append((RSA, k["der"], sig, m))
    got, mv = both(e, reg, rows, 32)
    return {"status": got, "moved": [list(x) for x in mv], "model": [bc.verify(r[1], r[2], r[3]) for r in rows]}


def main_launch_loop():
    from corda_amd.engine import Engine
    with Engine(1) as e:
        print(json.dumps(launch_loop_results(e)))


def test_rsa_launch_loop_small_workspace_subprocess():
    assert "CORDAHIP_RSA_WS_ROWS" not in os.environ
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import conftest; import test_gpu_sig_device_route as t; "
            "t.main_launch_loop()" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CORDAHIP_RSA_WS_ROWS="64"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    c = json.loads(r.stdout.strip().splitlines()[-1])
    assert c["status"] == c["model"] and {bc.OK, bc.BAD_SIG} <= set(c["status"])
    # the even rows and rows 63, 65, 127, 129 (both sides of the launch edges) are on the registered key
    assert c["moved"] == [[0, 0], [0, 0], [69, 61]]


# ---- 4. adversarial ranges ----------------------------------------------------------------------------
def test_overlapping_key_ranges_with_routing_on(eng, reg):
    """K23's overlapping-ranges batch (every even lane over the SAME key bytes, every odd lane reversed)
    with that key registered: the class holds key_bytes / 131 = 2 rows, the count the route pass reads
    is clipped to them, and every lane answers what it answers unrouted."""
    k = by_class(load_keys(), 64)[0]
    assert (k["n"], k["e"]) in reg.rsa
    n = 600
    rows = []
    for i in range(n):
        m, sig = pooled(k, i // 2, flip=i % 8 == 6)
        rows.append((RSA, k["der"] if i == 0 else b"", sig, m))
    ln = len(k["der"])
    res = []
    try:
        for dev_on in (False, True):
            switches(eng, ALL, dev_on)
            b0 = stats(eng)
            d = Dev(rows, 32, tail=256)
            assert d.key_bytes == ln and ln // 131 == 2
            d.ko = np.array([0 if i % 2 == 0 else ln for i in range(n + 1)], np.int64)
            d.run(eng)
            d.torch.cuda.synchronize()
            res.append((d.result(), d.verdict_bits(), moved(b0, stats(eng))))
            assert (d.key.cpu().numpy()[d.key_bytes:] == 0xA5).all()
    finally:
        switches(eng, (False,) * 3, False)
    want = [BAD_RANGE] * n
    for i in (0, 2):
        want[i] = bc.verify(k["der"], rows[i][2], rows[i][3])
    assert res[0][0] == res[1][0] == want and res[0][1] == res[1][1]
    assert res[0][2] == ((0, 0),) * 3 and res[1][2] == ((0, 0), (0, 0), (2, 0))
    sub = rsa_rows(60)  # the scratch is sound afterwards
    both(eng, reg, sub, 32)


def test_bad_ranges_with_canaries_and_routing_on(eng, mix, reg):
    rows, groups = mix
    sub = [rows[i] for i in groups[32][:200]]
    n = len(sub)
    a, c = 77, 140
    res = []
    try:
        for dev_on in (False, True):
            switches(eng, ALL, dev_on)
            d = Dev(sub, 32, msg_row=list(range(n)), tail=4096)
            d.ko, d.so = d.ko.copy(), d.so.copy()
            d.ko[a] = d.ko[a + 1] + 5   # a reversed key range (lane a - 1 gets a longer key)
            d.so[n] = d.sig_bytes + 100  # the last lane's signature reaches past sig_bytes
            mr = list(range(n))
            mr[c] = n                    # msg_row >= msg_rows
            d.msg_row = d.torch.from_numpy(np.asarray(mr, np.int32)).to(d.key.device)
            d.run(eng)
            d.torch.cuda.synchronize()
            kb, sb = d.key.cpu().numpy(), d.sig.cpu().numpy()
            assert (kb[d.key_bytes:] == 0xA5).all() and (sb[d.sig_bytes:] == 0xA5).all()
            res.append((d.result(), d.verdict_bits()))
    finally:
        switches(eng, (False,) * 3, False)
    assert res[0] == res[1] and all(res[1][0][i] == BAD_RANGE for i in (a, c, n - 1))
    assert res[1][0].count(_lib.OK) > 50


# ---- 5. ordering ----------------------------------------------------------------------------------------
def test_two_enqueues_on_one_stream_without_a_sync(eng, mix, reg):
    import torch
    rows, groups = mix
    big = [rows[i] for i in groups[32]]
    small = [rows[i] for i in groups[64][:97]]
    ed_only = [r for r in big if r[0] == ED][:333]
    want = [run_rows(eng, big, 32)[0], run_rows(eng, small, 64, is_valid=True, rsa=False)[0],
            run_rows(eng, ed_only, 32)[0]]
    s = torch.cuda.Stream()
    devs = [Dev(big, 32), Dev(small, 64), Dev(ed_only, 32)]
    torch.cuda.synchronize()
    try:
        switches(eng, ALL, True)
        b0 = stats(eng)
        with torch.cuda.stream(s):
            devs[0].run(eng, stream=s)
            devs[1].run(eng, is_valid=True, rsa=False, stream=s)
            devs[2].run(eng, stream=s)
        s.synchronize()
        mv = moved(b0, stats(eng))
    finally:
        switches(eng, (False,) * 3, False)
    assert [d.result() for d in devs] == want
    for d in devs:
        assert d.verdict_bits() == [int(g == 0) for g in d.result()]
    sums = [rule_counts(big, reg), rule_counts(small, reg, True, False), rule_counts(ed_only, reg)]
    assert mv == tuple(tuple(sum(x[f][j] for x in sums) for j in range(2)) for f in range(3))


def test_remove_right_behind_an_enqueue(eng, mix, reg):
    """vkey_remove waits for the routed batch before it clears the record the batch's rows matched"""
    import torch
    rows, groups = mix
    big = [rows[i] for i in groups[32]]
    want = run_rows(eng, big, 32)[0]
    extra = [r[1] for r in big if r[0] == ED and len(r[1]) == 32 and r[1] not in reg.ed][0]
    mine = Reg()
    mine.ed, mine.ec, mine.rsa = set(reg.ed) | {extra}, reg.ec, reg.rsa
    kid, st = eng.vkey_add_ed25519(extra)
    assert st == _lib.OK
    removed = False
    try:
        switches(eng, ALL, True)
        b0 = stats(eng)
        s = torch.cuda.Stream()
        d = Dev(big, 32)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d.run(eng, stream=s)
        eng.vkey_remove(kid)
        removed = True
        s.synchronize()
        assert d.result() == want
        assert moved(b0, stats(eng)) == rule_counts(big, mine)
        # and the key is gone: the next batch counts its rows generic
        b1 = stats(eng)
        assert run_rows(eng, big, 32)[0] == want
        assert moved(b1, stats(eng)) == rule_counts(big, reg)
    finally:
        switches(eng, (False,) * 3, False)
        if not removed:
            eng.vkey_remove(kid)


# ---- 6. the signed-transaction calls --------------------------------------------------------------------
def _register_signers(e, sigs, base):
    """beside the keys of `base`, which stay live: the most frequent Ed25519 signer (the notary's
    place) and one party's key of each other family; ids: the keys added here"""
    flat = [x for per in sigs for x in per]
    r = Reg()
    r.ed, r.ec, r.rsa = set(base.ed), set(base.ec), set(base.rsa)
    ed_keys = [x[1] for x in flat if x[0] == ED and len(x[1]) == 32]
    top = max(sorted(set(ed_keys)), key=ed_keys.count)
    if top not in r.ed:
        r.add_ed(e, top)
    pk = [x for x in flat if x[0] in (2, 3) and len(x[1]) == 65][0]
    if (pk[0], pk[1]) not in r.ec:
        r.add_ec(e, pk[0], pk[1])
    der = [x[1] for x in flat if x[0] == RSA and not isinstance(bc.decode_key(x[1]), int)][0]
    if bc.decode_key(der) not in r.rsa:
        kid, st = e.vkey_add_rsa(der)[:2]
        assert st == _lib.OK
        r.rsa.add(bc.decode_key(der))
        r.ids[(RSA, der)] = kid
    return r


def _tx_both(e, call):
    """call() with the device switch off and on: byte-identical outputs, every family's counters moved"""
    try:
        switches(e, ALL, False)
        b0 = stats(e)
        off = call()
        assert stats(e) == b0
        switches(e, ALL, True)
        on = call()
        mv = moved(b0, stats(e))
    finally:
        switches(e, (False,) * 3, False)
    for x, y in zip(on, off):
        assert x.tobytes() == y.tobytes()
    assert all(k > 0 for k, _ in mv), mv
    return off, mv


def test_signed_tx_calls_routed_are_byte_identical(eng, oracle, mix, reg):
    import torch
    dev = torch.device("cuda:0")
    rows, groups = mix
    pool = [rows[i] for i in groups[32]]
    rng = random.Random(53)
    ntx = 200
    txs = [[bytes(rng.getrandbits(8) for _ in range(rng.choice((33, 150)))) for _ in range(rng.choice((1, 2, 3)))]
           for _ in range(ntx)]
    ids, _ = eng.tx_ids(txs)
    sigs = _mixed_sigs(oracle, [ids[t].tobytes() for t in range(ntx)], pool)
    leaves = [x for tx in txs for x in tx]
    lb = torch.from_numpy(np.frombuffer(b"".join(leaves), np.uint8).copy()).to(dev)
    lo = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in leaves])]).astype(np.int64)).to(dev)
    tlo = torch.from_numpy(np.concatenate([[0], np.cumsum([len(tx) for tx in txs])]).astype(np.int64)).to(dev)
    r = _register_signers(eng, sigs, reg)
    eng.set_rsa_on_device(True)
    try:
        def call():
            tso, sg, outs, nsig = _dev_sig_args(torch, dev, sigs)
            eng.signed_tx_verify_device(lb, lo, tlo, tso, *sg, *outs)
            torch.cuda.synchronize()
            return _results(outs, ntx, nsig)
        off, mv = _tx_both(eng, call)
        flat = [(x[0], x[1], x[2], bytes(32)) for per in sigs for x in per]
        assert mv == rule_counts(flat, r)
        assert (off[1] == 0).sum() > ntx // 3 and (off[3] == _lib.BAD_SIG).sum() > 5
        # the component form, over the payment corpus
        name, blob, items, tio, cids, _ = next(iter(_comp_corpora(eng, oracle)))
        csigs = _mixed_sigs(oracle, cids, pool, every=7)
        off, mv = _tx_both(eng, lambda: _dev_comp(eng, torch, dev, blob, items, tio, csigs))
        cflat = [(x[0], x[1], x[2], bytes(32)) for per in csigs for x in per]
        assert mv == rule_counts(cflat, r) and [x.tobytes() for x in off[0]] == cids
    finally:
        eng.set_rsa_on_device(False)
        for kid in r.ids.values():
            eng.vkey_remove(kid)
