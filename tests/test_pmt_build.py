"""FilteredTransaction build (cordahip_filtered_tx_build), the CPU side: the
golden vectors regenerate from the oracle and are tear-offs the oracle's
verify accepts, the binding's struct, constants and slot bound agree with the
header and the oracle."""
import ctypes
import hashlib
import json
import os
import random
import re
import shutil
import subprocess

import pytest

import partial_merkle as pm
from corda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pmt_build_vectors.json")
H = lambda b: hashlib.sha256(b).digest()  # noqa: E731


@pytest.fixture(scope="module")
def cases():
    return json.load(open(GOLDEN))["cases"]


def test_golden_regenerates_from_the_oracle():
    import make_pmt_build_vectors as g
    assert g.dumps(g.generate()) == open(GOLDEN).read()
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_golden_covers_the_cases(cases):
    by = {c["name"]: c for c in cases}
    assert by["aaa_first"]["status"] == 12 and by["aaa_all"]["status"] == 0
    assert by["eight_dup_one"]["status"] == 12 and by["eight_dup_both"]["status"] == 0
    assert by["no_leaves"]["status"] == 6 and by["no_leaves"]["tokens"] == []
    assert by["ref_none"]["tokens"] == [[1, by["ref_none"]["root"]]]
    assert by["one_flagged"]["tokens"] == [[0, by["one_flagged"]["root"]]]
    assert by["one_unflagged"]["tokens"] == [[1, by["one_unflagged"]["root"]]]
    # 32 fully flagged reaches its slot bound; 33 has a 127-token slot, of which the oracle's tree
    # uses 75 (the 31 padding positions are cut into 5 Leaf(Z_j) tokens)
    assert all(by["full_%d" % m]["include"] == [1] * m for m in (32, 33))
    assert len(by["full_32"]["tokens"]) == 63 == _lib.pmt_slot_bound(32)
    assert len(by["full_33"]["tokens"]) == 75 and _lib.pmt_slot_bound(33) == 127
    assert sorted(len(by["random_m%d" % m]["leaves"]) for m in range(1, 35)) == list(range(1, 35))
    assert len(by["thousand_ends"]["leaves"]) == 1000 and sum(by["thousand_ends"]["include"]) == 2
    assert {c["status"] for c in cases} == {0, 6, 12}


def test_oracle_verify_accepts_every_built_tree(cases):
    n = 0
    for c in cases:
        if c["status"] != 0:
            assert c["tokens"] == []
            continue
        leaves = [bytes.fromhex(x) for x in c["leaves"]]
        toks = [(t, bytes.fromhex(h) if h else None) for t, h in c["tokens"]]
        flagged = [H(x) for x, f in zip(leaves, c["include"]) if f]
        assert pm.verify_tokens(toks, bytes.fromhex(c["root"]), flagged) is True, c["name"]
        assert len(toks) <= _lib.pmt_slot_bound(len(leaves)), c["name"]
        n += 1
    assert n > 30


def test_struct_layout_matches_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    cname, cls = "cordahip_filtered_build_batch", _lib.FilteredBuildBatch
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cordahip.h"', "int main(void) {",
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 14 * 8
    for f in cls._fields_:
        assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_status_constants_match_header():
    src = open(HEADER).read()
    vals = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define CORDAHIP_TX_(\w+) (\d+)", src))
    assert vals["HASHES_NOT_IN_TREE"] == _lib.TX_HASHES_NOT_IN_TREE == 12
    assert vals["TOK_SLOT_TOO_SMALL"] == _lib.TX_TOK_SLOT_TOO_SMALL == 13
    assert vals["NO_LEAVES"] == _lib.TX_NO_LEAVES == 6
    from corda_amd import resolve
    assert resolve.TX_HASHES_NOT_IN_TREE == 12
    assert len(set(vals.values())) == len(vals)  # no two tx statuses share a value
    for f in ("cordahip_filtered_tx_build", "cordahip_filtered_tx_build_submit", "cordahip_filtered_tx_build_device"):
        assert f in _lib.EXPORTS


def test_slot_bound_against_the_oracle():
    """2 * pad(m) - 1 is never exceeded by the oracle's trees and is reached when all of a
    power-of-two m is flagged."""
    assert [_lib.pmt_slot_bound(m) for m in (0, 1, 2, 3, 4, 5, 8, 9, 1000)] == [0, 1, 3, 7, 7, 15, 15, 31, 2047]
    rng = random.Random(39)
    for m in range(1, 40):
        hs = [H(b"slot-%d-%d" % (m, i)) for i in range(m)]
        tree = pm.merkle_tree(hs)
        worst = 0
        for mask in ([True] * m, [False] * m, *([rng.random() < p for _ in range(m)] for p in (0.2, 0.5, 0.8))):
            n = len(pm.tokens(pm.build(tree, [h for h, f in zip(hs, mask) if f])))
            assert n <= _lib.pmt_slot_bound(m), (m, mask)
            worst = max(worst, n)
        if m & (m - 1) == 0:
            assert worst == _lib.pmt_slot_bound(m) == 2 * m - 1
