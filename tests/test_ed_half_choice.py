"""Which lattice vector the Ed25519 prep hands to the ladder
(corda_amd/csrc/ed25519_half.hpp half_choose) on the host under AddressSanitizer
+ UBSan: tools/ed_half_check.cpp reads Euclid states and prints the chosen
(c0, c1); the big-integer model (tools/proto/half_scalar_windows.py) must choose
the same vector, candidate for candidate and tie for tie, with
c0 == c1 h (mod 8L) and c1 odd and positive. States: h = 0, 1, values below
sqrt(8L), L - 1 and its neighbours (cofactor -8, remainder 8 k), h with a tiny
even cofactor and a remainder of any size, h whose first short remainder is tiny
(1 .. 2^40) under an even cofactor of ~2^126 (the next Euclid vector is then
~2^250 long and its quotient needs the division step's wide path), and 10^5
seeded uniform h < L. On the seeded set the fraction of lanes that need more
than 65 ladder windows stays at the model's figure."""
import importlib.util
import math
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("half_scalar_windows",
                                               os.path.join(ROOT, "tools", "proto", "half_scalar_windows.py"))
hw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(hw)

L, M, T = hw.L, hw.M, hw.T
N_RANDOM = 100000
MASK = (1 << 256) - 1


def _tiny_rc_even_tc(rng, count):
    """h < L whose first remainder below sqrt(8L) is 2 r' (tiny) with the even cofactor 2 t':
    t' h == r' (mod 4L); r' t' << L makes (2 r', 2 t') a convergent's vector"""
    out = []
    while len(out) < count:
        t = rng.randrange(1 << 124, 1 << 126) | 1
        r = rng.randrange(1, 1 << rng.choice([1, 2, 8, 20, 40])) | 1
        h = r * pow(t, -1, 4 * L) % (4 * L)
        if h >= L:
            continue
        rp, rc, tp, tc = hw.euclid_state(h)
        if rc == 2 * r and abs(tc) == 2 * t:
            out.append(h)
    return out


def _tiny_even_tc(rng, count):
    """h < L with 8L = q h + r for a small even q: the cofactor is -q, the remainder r of any size below sqrt(8L)"""
    out = []
    while len(out) < count:
        q = 2 * rng.randrange(4, 40)
        r = rng.randrange(1, 1 << rng.choice([3, 30, 90, 127]))
        r += (M - r) % q
        h = (M - r) // q
        rp, rc, tp, tc = hw.euclid_state(h)
        if h < L and rc == r and tc == -q and r < T:
            out.append(h)
    return out


def _cases():
    rng = random.Random(20261020)
    edge = [0, 1, 2, 3, 8, T - 1, T - 2, (T - 1) // 2, 1 << 100, L - 1, L - 2, L - 3, L - 8, L - 1000]
    edge += _tiny_rc_even_tc(rng, 40) + _tiny_even_tc(rng, 40)
    return edge, [rng.randrange(L) for _ in range(N_RANDOM)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_choice_matches_big_integer_model_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ed_half_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_half_check.cpp")])
    edge, rnd = _cases()
    hs = edge + rnd
    states = [hw.euclid_state(h) for h in hs]
    # the edge set holds what it is meant to: even cofactors with tiny remainders / tiny cofactors
    ev = [s for s in states[:len(edge)] if s[3] % 2 == 0]
    assert sum(s[1] < (1 << 41) and abs(s[3]) > (1 << 120) for s in ev) >= 40
    assert sum(abs(s[3]) < 100 for s in ev) >= 40
    text = "".join("%064x %064x %064x %064x\n" % tuple(v & MASK for v in s) for s in states)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(hs)
    above = 0
    for k, (h, s, line) in enumerate(zip(hs, states, lines)):
        neg, c0abs, c1 = line.split()
        c0, c1 = (-1 if neg == "1" else 1) * int(c0abs, 16), int(c1, 16)
        assert (c0, c1) == hw.choose_state(*s), (h, c0, c1)
        assert (c0 - c1 * h) % M == 0 and c1 % 2 == 1 and c1 > 0, h
        if k >= len(edge):
            above += hw.windows((c0, c1)) > 65
    # the model's 128,000-lane run has 4.3 % of the lanes above 65 windows; both that
    # run and this one are binomial samples: four standard deviations of their difference
    p0 = 0.043
    margin = 4 * math.sqrt(p0 * (1 - p0) * (1 / N_RANDOM + 1 / 128000))
    frac = above / N_RANDOM
    print("lanes above 65 windows: %.4f (bound %.4f)" % (frac, p0 + margin))
    assert frac <= p0 + margin, (frac, p0 + margin)
