"""CPU check of the generated GF(2^255-19) asm blocks (corda_amd/csrc/fe25519_asm.hpp).

The header must equal tools/gen_fe_asm.render(). Every block (fe_mul2/3/4,
fe_sq2/4 in both operand schemes, fe_mul3x/4x, the chain block fe_sqsq2) is
emulated instruction by instruction on exact integers: a 32-bit result that
wraps (a scaled operand above 2^32) is an error, and so is a 64-bit column at
or above 2^64. The limbs are compared with a Python restatement of
fe25519.hpp's fe_mul / fe_sq (carry-chained columns, then fe_fold_top) and the
value with the product mod p. Operands: 0, 1, every limb at the tight bound,
every limb at the loose bound (3.3 x tight; 5 x tight for a multiply's
f-operand) and 200 random operands within the loose bounds. The GPU-side
bit-identity check is tools/microbench/fe_asm_check.hip.
"""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "corda_amd", "csrc", "fe25519_asm.hpp")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fe_asm  # noqa: E402

P = (1 << 255) - 19
M32 = (1 << 32) - 1
M26 = (1 << 26) - 1
M25 = (1 << 25) - 1
# fe25519.hpp's documented bounds
TIGHT = [(1 << 26) + (1 << 10) if i % 2 == 0 else (1 << 25) + (1 << 17) for i in range(10)]
LOOSE = [int(3.3 * t) for t in TIGHT]   # odd limbs: 111,162,163
LOOSE_F = [5 * t for t in TIGHT]        # fe_mul's f-operand
N_RANDOM = 200


def bits(k):
    return 25 if k & 1 else 26


def value(limbs):
    w, v = 0, 0
    for i, x in enumerate(limbs):
        v += x << w
        w += bits(i)
    return v


# ---------------------------------------------------------------------------
# restatement of fe25519.hpp
def fold_top(o, c):
    t = o[0] + c * 19
    assert t < 1 << 64
    o = list(o)
    o[0] = t & M26
    o[1] += t >> 26
    assert o[1] <= M32
    return o


def columns(terms):
    """carry-chained columns of the 10 term lists -> limbs, then fe_fold_top"""
    o, c = [], 0
    for k in range(10):
        acc = c
        for a, b in terms[k]:
            assert a <= M32 and b <= M32, "32-bit operand wraps"
            acc += a * b
        assert acc < 1 << 64, "column out of range"
        o.append(acc & (M25 if k & 1 else M26))
        c = acc >> bits(k)
    return fold_top(o, c)


def fe_mul_model(f, g):
    terms = []
    for k in range(10):
        col = []
        for i in range(10):
            j = (k - i) % 10
            a = f[i] * (2 if (i & 1) and (j & 1) else 1)
            b = g[j] * (19 if i + j >= 10 else 1)
            col.append((a, b))
        terms.append(col)
    return columns(terms)


def fe_sq_model(f, scaled13=True):
    """fe_sq: the 13-operand scheme (FE_SQ_SCALED13) or the 19-operand one"""
    terms = []
    for k in range(10):
        col = []
        for i in range(10):
            j = (k - i) % 10
            if j < i:
                continue
            wrap, oo = i + j >= 10, (i & 1) and (j & 1)
            if not scaled13:
                a = f[i] * (2 if i < j else 1) * (2 if oo else 1)
                b = f[j] * (19 if wrap else 1)
            elif i == j:
                a, b = f[i], f[j] * (19 if wrap else 1) * (2 if oo else 1)
            elif j & 1:
                a = f[i] * (2 if oo or not wrap else 1)
                b = f[j] * (38 if wrap else (2 if oo else 1))
            else:
                a, b = 2 * f[i], f[j] * (19 if wrap else 1)
            col.append((a, b))
        terms.append(col)
    return columns(terms)


# ---------------------------------------------------------------------------
# the header, parsed and emulated
def parse_header(text):
    """{(function name, variant): (asm lines, {operand: C expression}, C epilogue)};
    variant 1 is the #if FE_SQ_SCALED13 branch (and every unconditional block)."""
    funcs = {}
    variant = 1
    pos = 0
    rx = re.compile(r"^#if FE_SQ_SCALED13$|^#else$|^#endif$|"
                    r"CDEV void (fe_\w+)\([^)]*\) \{\n(.*?)  asm\(\n(.*?)\n      : (.*?)\n      :(.*?)\n      : "
                    r"[^\n]*\);\n(.*?)\}\n", re.S | re.M)
    for m in rx.finditer(text, pos):
        if m.group(1) is None:
            variant = {"#if FE_SQ_SCALED13": 1, "#else": 0, "#endif": 1}[m.group(0)]
            continue
        name, _, body, outs, ins, epi = m.groups()
        lines = [l.strip()[1:-3] for l in body.split("\n")]
        ops = {}
        for o in re.finditer(r'\[(\w+)\] "[=+&]*v"\(([^)]*)\)', outs + "," + ins):
            ops[o.group(1)] = o.group(2)
        funcs[(name, variant)] = (lines, ops, epi)
    return funcs


def emulate(lines, ops, inputs):
    """Run one asm body on exact integers. inputs: {C expression: value} for the
    operands read before they are written. Returns {C expression: value}."""
    vals = {n: inputs[e] for n, e in ops.items() if e in inputs}
    reg = {}  # the fixed VGPRs v160..v167, 32 bits each

    def pair(x):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", x)
        return ("v" + m.group(1), "v" + m.group(2)) if m else None

    def val(x):
        if x.startswith("%["):
            return vals[x[2:-1]]
        if pair(x):
            lo, hi = pair(x)
            return reg[lo] | (reg[hi] << 32)
        if re.fullmatch(r"v\d+", x):
            return reg[x]
        return int(x, 0)

    def put(x, v, width=32):
        assert 0 <= v < 1 << width, "%d-bit result out of range: %s" % (width, x)
        if x.startswith("%["):
            vals[x[2:-1]] = v
        elif pair(x):
            lo, hi = pair(x)
            reg[lo], reg[hi] = v & M32, v >> 32
        else:
            assert re.fullmatch(r"v\d+", x), x
            reg[x] = v

    for line in lines:
        op, rest = line.split(" ", 1)
        x = [t.strip() for t in rest.split(",")]
        if op == "v_mad_u64_u32":
            assert x[1] == "vcc"
            a, b = val(x[2]), val(x[3])
            assert a <= M32 and b <= M32
            put(x[0], a * b + val(x[4]), 64)
        elif op == "v_mul_lo_u32":      # exact: a scaled operand must not wrap
            put(x[0], val(x[1]) * val(x[2]))
        elif op == "v_mul_u32_u24":
            a, b = val(x[1]), val(x[2])
            assert a < 1 << 24 and b < 1 << 24
            put(x[0], a * b)
        elif op == "v_add_u32":
            put(x[0], val(x[1]) + val(x[2]))
        elif op == "v_lshlrev_b32":
            put(x[0], val(x[2]) << int(x[1]))
        elif op == "v_and_b32":
            put(x[0], val(x[1]) & val(x[2]) & M32)
        elif op == "v_lshrrev_b64":
            # a 64-bit operand (a carry) or a fixed pair
            v = val(x[2]) >> int(x[1])
            if x[0].startswith("%["):
                vals[x[0][2:-1]] = v
            else:
                put(x[0], v, 64)
        else:
            raise AssertionError("unexpected instruction " + op)
    return {e: vals[n] for n, e in ops.items() if n in vals}


def run_block(funcs, name, variant, operands):
    """operands: {"f0": limbs, "g0": limbs, ...} -> {"r0": limbs, ...} after the C epilogue"""
    lines, ops, epi = funcs[(name, variant)]
    inputs = {"%s.v[%d]" % (nm, k): limbs[k] for nm, limbs in operands.items() for k in range(10)}
    out = emulate(lines, ops, inputs)
    res = {}
    for m in re.finditer(r"fe_fold_top\((\w+), (\w+)\);", epi):
        o, c = m.groups()
        res[o] = fold_top([out["%s.v[%d]" % (o, k)] for k in range(10)], out[c])
    ret = {}
    for m in re.finditer(r"  (r\d) = (o\d);", epi):
        ret[m.group(1)] = res[m.group(2)]
    if not ret:  # in-place block: the read-write operands
        for nm in operands:
            ret[nm] = [out["%s.v[%d]" % (nm, k)] for k in range(10)]
    return ret


def operand_sets(bound, rng):
    """0, 1, tight, the bound itself, then random operands within it"""
    yield [0] * 10
    yield [1] + [0] * 9
    yield list(TIGHT)
    yield list(bound)
    for _ in range(N_RANDOM):
        yield [rng.randint(0, b) for b in bound]


@pytest.fixture(scope="module")
def funcs():
    with open(HDR) as f:
        return parse_header(f.read())


def test_header_is_generated():
    with open(HDR) as f:
        assert f.read() == gen_fe_asm.render(), "re-run tools/gen_fe_asm.py"


def test_every_block_is_parsed(funcs):
    assert set(funcs) == {("fe_mul2", 1), ("fe_mul3", 1), ("fe_mul4", 1), ("fe_sq2", 1), ("fe_sq2", 0),
                          ("fe_sq4", 1), ("fe_sq4", 0), ("fe_sqsq2", 1), ("fe_mul3x", 1), ("fe_mul4x", 1)}


def test_sq_models_agree():
    """both operand schemes give the same limbs, equal to f^2 mod p"""
    rng = random.Random(13)
    for f in operand_sets(LOOSE, rng):
        want = fe_sq_model(f, True)
        assert want == fe_sq_model(f, False)
        assert value(want) % P == value(f) ** 2 % P
        assert all(x <= t for x, t in zip(want, TIGHT))


def test_scaled13_operands_and_counts(funcs):
    """13 scaling instructions per chain: f2_0..7 and 38 f5, 19 f6, 38 f7, 19 f8, 38 f9"""
    for name, n in (("fe_sq2", 2), ("fe_sq4", 4), ("fe_sqsq2", 4)):
        lines = funcs[(name, 1)][0]
        adds = [l for l in lines if l.startswith("v_add_u32 %[f2_")]
        muls = [l for l in lines if l.startswith("v_mul_lo_u32")]
        assert len(adds) == 8 * n and len(muls) == 5 * n
        assert sorted({re.match(r"v_mul_lo_u32 %\[(f\d+_\d)", l).group(1) for l in muls}) == [
            "f19_6", "f19_8", "f38_5", "f38_7", "f38_9"]
        assert not any(l.startswith("v_lshlrev") or "f4_" in l for l in lines)
    assert 38 * LOOSE[1] < 1 << 32 and 38 * 113025455 < 1 << 32 <= 38 * 113025456


@pytest.mark.parametrize("n", [2, 3, 4])
def test_mul_blocks(funcs, n):
    rng = random.Random(100 + n)
    fs = [list(operand_sets(LOOSE_F, rng)) for _ in range(n)]
    gs = [list(operand_sets(LOOSE, rng)) for _ in range(n)]
    for it in range(len(fs[0])):
        ops = {}
        for p in range(n):
            q = (it + p) % len(fs[0]) if it >= 4 else it  # edge operands in every chain at once
            ops["f%d" % p], ops["g%d" % p] = fs[p][q], gs[p][q]
        got = run_block(funcs, "fe_mul%d" % n, 1, ops)
        for p in range(n):
            want = fe_mul_model(ops["f%d" % p], ops["g%d" % p])
            assert got["r%d" % p] == want
            assert value(want) % P == value(ops["f%d" % p]) * value(ops["g%d" % p]) % P


@pytest.mark.parametrize("n", [3, 4])
def test_outer_blocks(funcs, n):
    rng = random.Random(200 + n)
    sets = [list(operand_sets(b, rng)) for b in (LOOSE_F, LOOSE_F, LOOSE, LOOSE)]
    pairs = (("f0", "g0"), ("f1", "g1"), ("f0", "g1"), ("f1", "g0"))[:n]
    for it in range(len(sets[0])):
        ops = {nm: sets[i][it] for i, nm in enumerate(("f0", "f1", "g0", "g1"))}
        got = run_block(funcs, "fe_mul%dx" % n, 1, ops)
        for p, (f, g) in enumerate(pairs):
            want = fe_mul_model(ops[f], ops[g])
            assert got["r%d" % p] == want
            assert value(want) % P == value(ops[f]) * value(ops[g]) % P


@pytest.mark.parametrize("variant", [1, 0], ids=["scaled13", "scaled19"])
@pytest.mark.parametrize("n", [2, 4])
def test_sq_blocks(funcs, n, variant):
    rng = random.Random(300 + n)
    fs = [list(operand_sets(LOOSE, rng)) for _ in range(n)]
    for it in range(len(fs[0])):
        ops = {"f%d" % p: fs[p][it] for p in range(n)}
        got = run_block(funcs, "fe_sq%d" % n, variant, ops)
        for p in range(n):
            want = fe_sq_model(ops["f%d" % p], bool(variant))
            assert got["r%d" % p] == want
            assert value(want) % P == value(ops["f%d" % p]) ** 2 % P


def test_chain_block(funcs):
    """fe_sqsq2 equals two restated squarings, each with its fold"""
    rng = random.Random(400)
    fs = [list(operand_sets(LOOSE, rng)) for _ in range(2)]
    for it in range(len(fs[0])):
        ops = {"f%d" % p: fs[p][it] for p in range(2)}
        got = run_block(funcs, "fe_sqsq2", 1, ops)
        for p in range(2):
            want = fe_sq_model(fe_sq_model(ops["f%d" % p]))
            assert got["f%d" % p] == want
            assert value(want) % P == pow(value(ops["f%d" % p]), 4, P)
