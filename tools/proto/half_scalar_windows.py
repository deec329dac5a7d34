"""Model of the Ed25519 ladder's window counts (dev tool and the big-integer
reference of tests/test_ed_half_choice.py and tests/test_gpu_ed_ladder_order.py).

The prep (ed25519.hip half_scalars) runs Euclid on (8L, h) to the first
remainder below sqrt(8L) and hands (rp, rc, tp, tc) to half_choose
(ed25519_half.hpp), which picks (c0, c1) with c0 == c1 h (mod 8L), c1 odd.
A lane then needs max((bitlen(max(|c0|, c1)) + 2) / 2, 61) ladder windows, and
a wave of 64 lanes runs its longest lane's count. `choose` below is that
selection rule, candidate for candidate and tie for tie; `choose_old` is the
rule before the previous Euclid vector v0 = (rp, tp) was considered.

    python tools/proto/half_scalar_windows.py [lanes] [seed] [--json]

prints the table of mean windows per lane and per wave for: the old rule, the
six-candidate rule, the true shortest odd-c1 vector, either rule with each
256-lane block's lanes handed to its four waves in window-count order, and a
global sort (the floor).
"""
import json
import math
import random
import sys

L = 2**252 + 27742317777372353535851937790883648493
M = 8 * L
T = math.isqrt(M) + 1
MIN_WINDOWS = 61  # the fixed-base digits of e over B need them (ed25519_sel.hpp kBMinWindows; 57 at 16-bit windows)


def euclid_state(h):
    """plain Euclid on (8L, h) until the current remainder drops below isqrt(8L) + 1"""
    rp, rc, tp, tc = M, h, 0, 1
    while rc >= T:
        q = rp // rc
        rp, rc = rc, rp - q * rc
        tp, tc = tc, tp - q * tc
    return rp, rc, tp, tc


def vec_bits(v):
    return max(abs(v[0]).bit_length(), abs(v[1]).bit_length())


def _norm(v):
    """c1 positive, as the record stores it"""
    return (-v[0], -v[1]) if v[1] < 0 else v


def candidates(rp, rc, tp, tc, six=True):
    """the candidates in the order half_choose tries them (tc even)"""
    q = rp // rc
    v0, v1, v3 = (rp, tp), (rc, tc), (rp - q * rc, tp - q * tc)
    out = [v3, (v1[0] + v3[0], v1[1] + v3[1]), (v1[0] - v3[0], v1[1] - v3[1])]
    if six:
        out += [v0, (v0[0] + v1[0], v0[1] + v1[1]), (v0[0] - v1[0], v0[1] - v1[1])]
    return out


def choose_state(rp, rc, tp, tc, six=True):
    if tc & 1:
        return _norm((rc, tc))
    best = None
    for v in candidates(rp, rc, tp, tc, six):
        if not v[1] & 1:  # parity guard; never taken: gcd(tp, tc) = 1
            continue
        if best is None or vec_bits(v) < vec_bits(best):  # first of the shortest wins
            best = v
    return _norm(best)


def choose(h):
    return choose_state(*euclid_state(h))


def choose_old(h):
    return choose_state(*euclid_state(h), six=False)


def choose_shortest(h):
    """the shortest odd-c1 vector of the lattice, by max bit length: Lagrange-reduce
    the basis (v1, v3), then every a b1 + b b2 with |a|, |b| <= 3"""
    rp, rc, tp, tc = euclid_state(h)
    if rc == 0:
        return _norm((rc, tc))
    q = rp // rc
    b1, b2 = (rc, tc), (rp - q * rc, tp - q * tc)
    n2 = lambda v: v[0] * v[0] + v[1] * v[1]  # noqa: E731
    if n2(b1) > n2(b2):
        b1, b2 = b2, b1
    while True:
        d = n2(b1)
        mu = (2 * (b1[0] * b2[0] + b1[1] * b2[1]) + d) // (2 * d)  # nearest integer
        b2 = (b2[0] - mu * b1[0], b2[1] - mu * b1[1])
        if n2(b2) >= n2(b1):
            break
        b1, b2 = b2, b1
    best = None
    for a in range(-3, 4):
        for b in range(-3, 4):
            v = (a * b1[0] + b * b2[0], a * b1[1] + b * b2[1])
            if v[1] & 1 and (best is None or vec_bits(v) < vec_bits(best)):
                best = v
    return _norm(best)


def windows(v):
    return max((vec_bits(v) + 2) // 2, MIN_WINDOWS)


def wave_mean(ws, sort_block=0):
    """mean over waves of 64 lanes of the wave's largest count; sort_block: lanes
    sorted by count inside blocks of that many lanes first"""
    if sort_block:
        ws = [w for i in range(0, len(ws), sort_block) for w in sorted(ws[i:i + sort_block])]
    mx = [max(ws[i:i + 64]) for i in range(0, len(ws), 64)]
    return sum(mx) / len(mx)


def table(n, seed):
    rng = random.Random(seed)
    hs = [rng.randrange(L) for _ in range(n)]
    rows = []
    for name, rule, block in (("today: v3, v1+-v3", choose_old, 0),
                              ("six candidates: v3, v1+-v3, v0, v0+-v1", choose, 0),
                              ("true shortest odd-c1 vector", choose_shortest, 0),
                              ("today's rule, block's lanes to its 4 waves in count order", choose_old, 256),
                              ("six candidates, block's lanes to its 4 waves in count order", choose, 256),
                              ("six candidates, global sort (floor)", choose, n)):
        ws = [windows(rule(h)) for h in hs]
        rows.append({"rule": name, "lane_mean": sum(ws) / n, "wave_mean": wave_mean(ws, block), "max": max(ws),
                     "frac_above_65": sum(w > 65 for w in ws) / n})
    return {"lanes": n, "seed": seed, "rows": rows}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    t = table(int(args[0]) if args else 256000, int(args[1]) if len(args) > 1 else 19)
    if "--json" in sys.argv:
        print(json.dumps(t))
    else:
        print("%d uniform h < L, seed %d, 64 lanes per wave" % (t["lanes"], t["seed"]))
        for r in t["rows"]:
            print("%-62s lane %.2f  wave %.2f  max %d  >65: %.2f %%" % (r["rule"], r["lane_mean"], r["wave_mean"],
                                                                     r["max"], 100 * r["frac_above_65"]))
