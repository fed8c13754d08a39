"""The reference of the key validation tests (csrc/validate.hpp, abi_validate.hip): plain Python integers.

    on_curve(P)     y^2 = x^3 + b, both coordinates below the modulus; the all-zero encoding is infinity
    in_subgroup(P)  r * P is None -- THE definition, for all four curves and for G2 of BLS12-381

and a seeded maker of adversarial points per curve.  The curve numbers are oracle/pyref.py's and tests/harness/ref377.py's (through
ref377's private copy, which holds all four curves), the ladder is harness/sw_setup.py's Jacobian one, Fq2 is harness/g2ref.py's; nothing
is taken from the code under test.

The cofactors h = (x - 1)^2 / 3 of the two BLS12 curves, factored (FACTORS, checked against the cofactor below):
    BLS12-381   3 * 11^2 * 10177^2 * 859267^2 * 52437899^2
    BLS12-377   2^92 * 3 * 7^2 * 13^2 * 499^2
For a prime l with l^2 | (x - 1)^2 the l-part of E(Fq) is (Z / l^(k/2))^2, not cyclic: a point T = (#E / l^k) * Q has order at most
l^(k/2) (l for the squared primes, 2^46 for BLS12-377's 2^92), and the torsion is two-dimensional -- so several Q per prime power are
taken, and for 2^92 every order 2^46, 2^45, .. 2 by doubling.  `torsion_order` computes the exact order of every such point, and
adversarial() asserts that for each prime power at least one point reaches the full exponent l^ceil(k/2) of its component.
"""
import ctypes as C
import functools
import random

import numpy as np

from harness import g2ref as G2
from harness import ref377
from harness import sw_setup as S

R = S.R
CURVES = S.CURVES
CURVE_ID = S.CURVE_ID
BLS12 = ("bls12_381", "bls12_377")
FACTORS = {"bls12_381": ((3, 1), (11, 2), (10177, 2), (859267, 2), (52437899, 2)),
           "bls12_377": ((2, 92), (3, 1), (7, 2), (13, 2), (499, 2))}
Q_PER_PRIME_POWER = 3

CHECK_ON_CURVE, CHECK_SUBGROUP = 1, 2      # PC_HIP_CHECK_* (include/pc_hip.h)


def P():
    return ref377.probe()


def order_r(curve):
    return R.curve_params(curve)[1]


def on_curve(curve, pt):
    return pt is R.INF or R.on_curve(curve, pt)


def in_subgroup(curve, pt):
    return S.mul(curve, order_r(curve), pt) is R.INF


def neg(curve, pt):
    return R.ec_neg(curve, pt)


def add(curve, a, b):
    return R.ec_add(curve, a, b)


def curve_point(curve, rnd):
    """a seeded point of the curve (of the whole group E(Fq): outside the subgroup with overwhelming probability where h != 1)"""
    p = S.field(curve)[0]
    while True:
        x = rnd.randrange(p)
        n = S.rhs(curve, x)
        if n and S.is_square(curve, n):
            y = S.sqrt(curve, n)
            return (x, y if rnd.random() < 0.5 else p - y)


def torsion_order(curve, l, T):
    """the e with l^e T = O, e minimal (T in the l-part)"""
    e = 0
    while T is not R.INF:
        T = S.mul(curve, l, T)
        e += 1
        assert e <= 128
    return e


# ---- the fast test of the two BLS12 curves, restated over integers (eprint 2021/1130 section 6) ---------------------------------------

def bls12_x(curve):
    """the curve parameter from the moduli: r = x^4 - x^2 + 1 and p = (x - 1)^2 r / 3 + x"""
    import math
    p, r, _ = R.curve_params(curve)
    d = math.isqrt(4 * r - 3)
    ax = math.isqrt((1 + d) // 2)
    assert ax ** 4 - ax ** 2 + 1 == r
    xs = [x for x in (ax, -ax) if (x - 1) ** 2 * r // 3 + x == p]
    assert len(xs) == 1 and (xs[0] - 1) ** 2 // 3 == S.cofactor(curve)
    return xs[0]


def phi_matches(curve, beta, pt):
    """(beta x, y) == -[x^2] (x, y)"""
    p = S.field(curve)[0]
    x = bls12_x(curve)
    return (beta * pt[0] % p, pt[1]) == neg(curve, S.mul(curve, x * x, pt))


# ---- adversarial points -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def adversarial(curve):
    """-> tuple of (kind, point).  BLS12: torsion points of every prime power of the cofactor (kind "torsion l^k"), G + T, members
    h * Q, pure torsion r * Q, raw curve points, the two points with x = 0, infinity, small multiples of the generator.  Cofactor 1: raw
    points, multiples of the generator, infinity."""
    p, r, b = R.curve_params(curve)
    h = S.cofactor(curve)
    G = R.generator(curve)
    rnd = random.Random(2021_1130 + CURVE_ID[curve])
    out = [("infinity", R.INF)] + [("generator multiple", S.mul(curve, k, G)) for k in (1, 2, 3, r - 1, r - 2, (r + 1) // 2)]
    raw = [curve_point(curve, rnd) for _ in range(8)]
    out += [("raw", q) for q in raw]
    if h != 1:
        n = h * r
        prod = 1
        for l, k in FACTORS[curve]:
            prod *= l ** k
        assert prod == h, "the factorization is not the cofactor's"
        for l, k in FACTORS[curve]:
            full = (k + 1) // 2
            reached = 0
            for _ in range(Q_PER_PRIME_POWER):
                T = S.mul(curve, n // l ** k, curve_point(curve, rnd))
                e = torsion_order(curve, l, T)
                reached = max(reached, e)
                while T is not R.INF:                               # T, l T, l^2 T, ..: every order l^e, .., l
                    out.append(("torsion %d^%d" % (l, k), T))
                    out.append(("G + T", add(curve, G, T)))
                    T = S.mul(curve, l, T)
            assert reached == full, "%s: no torsion point of order %d^%d (reached %d^%d)" % (curve, l, full, l, reached)
        out += [("member", S.mul(curve, h, q)) for q in raw[:4]]
        out += [("pure torsion", S.mul(curve, r, q)) for q in raw[:4]]
        y0 = S.sqrt(curve, b)
        out += [("x = 0", (0, y0)), ("x = 0", (0, p - y0))]
    assert all(on_curve(curve, q) for _, q in out)
    return tuple(out)


@functools.lru_cache(None)
def membership(curve):
    """in_subgroup of every adversarial point, with the conditions the tests rest on: members and non-members of every kind"""
    adv = adversarial(curve)
    want = tuple(1 if in_subgroup(curve, q) else 0 for _, q in adv)
    by_kind = {}
    for (kind, _), w in zip(adv, want):
        by_kind.setdefault(kind, set()).add(w)
    assert by_kind["infinity"] == {1} and by_kind["generator multiple"] == {1}
    if S.cofactor(curve) == 1:
        assert by_kind["raw"] == {1} and set(want) == {1}
    else:
        assert by_kind["raw"] == {0} and by_kind["member"] == {1} and by_kind["pure torsion"] == {0} and by_kind["x = 0"] == {0}
        assert by_kind["G + T"] == {0}
        for l, k in FACTORS[curve]:
            assert by_kind["torsion %d^%d" % (l, k)] == {0}
    return want


def point_words(curve, pt):
    return S.point_words(curve, pt)


def raw_words(curve, xraw, yraw):
    """two raw limb values (not reduced, not converted) as the 2 n words of a resident point"""
    n = S.field(curve)[2]
    assert 0 <= xraw < 1 << (32 * n) and 0 <= yraw < 1 << (32 * n)
    return [(c >> (32 * k)) & 0xffffffff for c in (xraw, yraw) for k in range(n)]


def want_on_curve_words(curve, words):
    """SwOnCurveBody's contract over raw words: all zero, or both limbs values below p and the Montgomery residues on the curve"""
    p, _, n = S.field(curve)
    w = [int(v) for v in words]
    if not any(w):
        return 1
    X, Y = (sum(v << (32 * k) for k, v in enumerate(w[h * n:(h + 1) * n])) for h in (0, 1))
    if X >= p or Y >= p:
        return 0
    return 1 if R.on_curve(curve, (S.unmont(curve, X), S.unmont(curve, Y))) else 0


@functools.lru_cache(None)
def on_curve_cases(curve):
    """-> tuple of (kind, words): every adversarial point (on the curve), and for three of them y + 1, the swapped coordinates, a
    coordinate equal to p, one equal to p + 1, and the point with p added to a coordinate (congruent to a point of the curve, but the
    limbs are not below p)"""
    p, _, n = S.field(curve)
    top = 1 << (32 * n)
    out = [("valid: " + kind, tuple(point_words(curve, q))) for kind, q in adversarial(curve)]
    real = [q for _, q in adversarial(curve) if q is not R.INF]
    picks = [real[0], real[len(real) // 2], real[-1]]          # the generator, a middle one, the last (x = 0 on the BLS12 curves)
    for x, y in picks:
        X, Y = S.mont(curve, x), S.mont(curve, y)
        if x or (y + 1) % p:                                    # ((0, -1) + (0, 1) would be the all-zero encoding of infinity)
            out.append(("y + 1", tuple(point_words(curve, (x, (y + 1) % p)))))
        out.append(("swapped", tuple(point_words(curve, (y, x)))))
        out.append(("x = p", tuple(raw_words(curve, p, Y))))
        out.append(("y = p", tuple(raw_words(curve, X, p))))
        out.append(("x = p + 1", tuple(raw_words(curve, p + 1, Y))))
        out.append(("y = p + 1", tuple(raw_words(curve, X, p + 1))))
        if X + p < top:
            out.append(("x + p", tuple(raw_words(curve, X + p, Y))))
        if Y + p < top:
            out.append(("y + p", tuple(raw_words(curve, X, Y + p))))
    out.append(("all ones", tuple([0xffffffff] * (2 * n))))
    want = [want_on_curve_words(curve, w) for _, w in out]
    kinds = {k.split(":")[0] for k, _ in out}
    assert {"valid", "y + 1", "swapped", "x = p", "y = p", "x = p + 1", "y = p + 1", "all ones"} <= kinds
    # (the swapped coordinates are left to the reference: on BLS12-377, b = 1, (0, -1) swapped is (-1, 0), the point of order 2)
    assert all(w == 1 for (k, _), w in zip(out, want) if k.startswith("valid")) and all(w == 0 for (k, _), w in zip(out, want) if not k.startswith(("valid", "swapped")))
    assert 0 in [w for (k, _), w in zip(out, want) if k == "swapped"]
    if curve in BLS12:      # x = p is the non-canonical zero: congruent to the order-3 point (0, sqrt(b)), which IS on the curve
        assert picks[-1][0] == 0 and ("x + p" in kinds or "y + p" in kinds)
    return tuple(out), tuple(want)


# ---- G2 of BLS12-381 ----------------------------------------------------------------------------------------------------------------

def g2_words(pt):
    return np.frombuffer(G2.point_bytes(pt), dtype=np.uint32).copy()


def g2_in_subgroup(pt):
    return G2.mul(G2.R, pt, mod_r=False) is G2.INF


def g2_twist_point(rnd):
    while True:
        x = (rnd.randrange(G2.P), rnd.randrange(G2.P))
        y = G2.f2_sqrt(G2.f2_add(G2.f2_mul(G2.f2_sqr(x), x), G2.B2))
        if y is not None:
            assert G2.on_twist((x, y))
            return (x, y)


@functools.lru_cache(None)
def g2_cases():
    """-> (kinds, words n x 48, on-curve flags, subgroup flags of the on-curve entries (None where off the curve))"""
    rnd = random.Random(381_2)
    g = G2.generator()
    members = [G2.mul(k, g) for k in (1, 2, 3, G2.R - 1, 0x1234567)]
    raws = [g2_twist_point(rnd) for _ in range(4)]
    kinds = ["infinity"] + ["member"] * len(members) + ["raw twist point"] * len(raws)
    pts = [G2.INF] + members + raws
    words = [g2_words(q) for q in pts]
    on = [1] * len(pts)
    sub = [1 if g2_in_subgroup(q) else 0 for q in pts]
    assert sub == [1] + [1] * len(members) + [0] * len(raws), "a raw twist point is a member (or a multiple of the generator is not)"
    x, y = members[0]
    off = [("y + 1", (x, G2.f2_add(y, (1, 0)))), ("swapped", (y, x)), ("G1's equation", ((R.generator("bls12_381")[0], 0), (R.generator("bls12_381")[1], 0)))]
    for kind, q in off:
        assert not G2.on_twist(q)
        kinds.append(kind); words.append(g2_words(q)); on.append(0); sub.append(None)
    for j in range(4):                                  # one coefficient of a member plus p: congruent, but not below the modulus
        w = g2_words(members[1]).reshape(4, 12)
        v = int.from_bytes(w[j].tobytes(), "little") + G2.P
        assert v < 1 << 384
        w[j] = np.frombuffer(v.to_bytes(48, "little"), dtype=np.uint32)
        kinds.append("coefficient %d + p" % j); words.append(w.reshape(-1)); on.append(0); sub.append(None)
    return tuple(kinds), np.array(words, dtype=np.uint32), tuple(on), tuple(sub)


# ---- the probe ------------------------------------------------------------------------------------------------------------------------

def host_probe():
    return P().host_probe()


def device_probe():
    return P().device_probe()


def twin(name, probe_, host, run):
    """run(library) -> flags; on the device the host build's must be the same"""
    out = run(probe_)
    if host is not probe_:
        P().same_words(name, out, run(host))
    return out


def run_flags(pr, entry, pre, words):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    flags = np.full(len(words), 0xdeadbeef, dtype=np.uint32)
    pr.call(entry, *pre, C.c_size_t(len(words)), P().p32(words), P().p32(flags))
    return flags


def check_on_curve(probe_, host, curve):
    cases, want = on_curve_cases(curve)
    words = np.array([w for _, w in cases], dtype=np.uint32)
    got = twin("validate on_curve " + curve, probe_, host, lambda pr: run_flags(pr, "pc_probe_validate_on_curve", (C.c_int(CURVE_ID[curve]),), words))
    bad = [(i, cases[i][0], int(got[i]), want[i]) for i in range(len(cases)) if int(got[i]) != want[i]]
    assert not bad, "%s on-curve flags (lane, kind, got, want): %s" % (curve, bad[:8])
    return len(cases)


def adversarial_words(curve):
    return np.array([point_words(curve, q) for _, q in adversarial(curve)], dtype=np.uint32)


def check_subgroup(probe_, host, curve, entry):
    """entry: pc_probe_validate_ladder or pc_probe_validate_fast, against in_subgroup on the whole adversarial set; returns the flags"""
    adv, want = adversarial(curve), membership(curve)
    words = adversarial_words(curve)
    got = twin("validate %s %s" % (entry, curve), probe_, host, lambda pr: run_flags(pr, entry, (C.c_int(CURVE_ID[curve]),), words))
    bad = [(i, adv[i][0], int(got[i]), want[i]) for i in range(len(adv)) if int(got[i]) != want[i]]
    assert not bad, "%s %s flags (lane, kind, got, want): %s" % (curve, entry, bad[:8])
    return got


def constants(probe_, curve):
    """the generated constants of the fast test -> (x, beta' as an integer, beta' is the GLV header's)"""
    n = S.field(curve)[2]
    out = np.zeros(4 + n, dtype=np.uint32)
    assert probe_.raw("pc_probe_validate_constants", C.c_int(CURVE_ID[curve]), P().p32(out)) == 0
    x = int(out[0]) | (int(out[1]) << 32)
    beta = S.unmont(curve, sum(int(v) << (32 * k) for k, v in enumerate(out[4:])))
    return (-x if out[2] else x), beta, bool(out[3])


def check_g2(probe_, host):
    kinds, words, on, sub = g2_cases()
    got_on = twin("validate g2 on_curve", probe_, host, lambda pr: run_flags(pr, "pc_probe_validate_g2", (C.c_int(0),), words))
    assert [int(f) for f in got_on] == list(on), "G2 on-curve flags %s, want %s (%s)" % (list(got_on), on, kinds)
    keep = [i for i, s in enumerate(sub) if s is not None]
    got = twin("validate g2 subgroup", probe_, host, lambda pr: run_flags(pr, "pc_probe_validate_g2", (C.c_int(1),), words[keep]))
    assert [int(f) for f in got] == [sub[i] for i in keep], "G2 subgroup flags %s, want %s" % (list(got), [sub[i] for i in keep])
    return len(kinds) + len(keep)


def check_tally(probe_, host):
    """ValidateTallyBody: the count, the lowest failing index and the bytes, for failures at the edges of a 256-lane block"""
    lanes = 0
    for n, bad in ((1, ()), (1, (0,)), (64, (63,)), (65, (64, 63)), (257, (256,)), (257, (255, 256, 0)), (1000, (999, 64, 255)), (1000, ())):
        flags = np.ones(n, dtype=np.uint32)
        flags[list(bad)] = 0

        def run(pr):
            ok, out = np.zeros((n + 3) // 4, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
            pr.call("pc_probe_validate_tally", C.c_size_t(n), P().p32(flags), P().p32(ok), P().p32(out))
            return np.concatenate([ok, out])
        got = twin("validate tally", probe_, host, run)
        assert int(got[-2]) == len(bad) and int(got[-1]) == (min(bad) if bad else 0xffffffff), (n, bad, got[-2:])
        assert list(got[:-2].view(np.uint8)[:n]) == [0 if i in bad else 1 for i in range(n)]
        lanes += n
    return lanes


# ---- keys for the ABI tests -------------------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 257, 1000)
EDGES = (0, -1, 63, 64, 255, 256)       # the wave and workgroup edges of a 256-lane block; -1: the last point


def plant_indices(n):
    return sorted({(n - 1 if e < 0 else e) for e in EDGES if (n - 1 if e < 0 else e) < n})


@functools.lru_cache(None)
def member_words(curve):
    """(i + 1) G for i < 1000 as resident words (read-only, shared: a test takes a prefix)"""
    pts = R.gen_bases(curve, max(SIZES))
    assert all(q is not R.INF for q in pts)
    w = np.array([point_words(curve, q) for q in pts], dtype=np.uint32)
    w.setflags(write=False)
    return w


@functools.lru_cache(None)
def non_member_words(curve):
    """one resident record per kind of non-member of the adversarial set, in a fixed order -- a torsion point per prime power first --
    checked by the reference to be on the curve and outside the subgroup"""
    seen, out = set(), []
    for (kind, q), w in zip(adversarial(curve), membership(curve)):
        if w == 0 and kind not in seen:
            seen.add(kind)
            out.append((kind, tuple(point_words(curve, q))))
    assert {"torsion %d^%d" % f for f in FACTORS[curve]} | {"G + T", "raw", "pure torsion", "x = 0"} == seen
    return tuple(out)


@functools.lru_cache(None)
def off_curve_words(curve):
    cases, want = on_curve_cases(curve)
    out = tuple((k, w) for (k, w), f in zip(cases, want) if f == 0)
    assert len(out) >= 6
    return out


def planted_key(curve, n, at, kind="subgroup", start=0):
    """n members with the entries `at` replaced, in turn, by the non-members (kind "subgroup"), by off-curve records ("on_curve") or
    alternately by both ("both") -> (words n x W, on-curve flags, flags of on-curve AND member)"""
    w = member_words(curve)[:n].copy()
    on, both = [1] * n, [1] * n
    pools = {"subgroup": [(0, non_member_words(curve))] if curve in BLS12 else [], "on_curve": [(1, off_curve_words(curve))]}
    pools["both"] = pools["subgroup"] + pools["on_curve"]
    for j, i in enumerate(at):
        off, pool = pools[kind][j % len(pools[kind])]
        w[i] = pool[(start + j // len(pools[kind])) % len(pool)][1]
        both[i] = 0
        if off:
            on[i] = 0
    return w, on, both


def windows(n, at):
    """(offset, count) windows that start and end on a planted index, the whole key, and the windows just inside them"""
    out = {(0, n)}
    for a in at:
        for b in at:
            if a <= b:
                out.add((a, b - a + 1))
                if b > a:
                    out.add((a + 1, b - a - 1))
    return sorted(out)


def expect_query(flags, offset, count):
    """(bad, first_bad or None, flags) of a window over the per-point expectations"""
    f = list(flags[offset:offset + count])
    bad = [i for i, v in enumerate(f) if not v]
    return len(bad), (bad[0] if bad else None), f


def upload_words(ctx, curve, words):
    """a resident key from n x W uint32 words"""
    import poly_commit_amd as pc
    return pc.Srs(ctx, curve, np.ascontiguousarray(words).view(np.uint64))


def query(key, offset, count, on_curve, subgroup):
    bad, first, flags = key.check(offset, count, on_curve=on_curve, subgroup=subgroup, want_flags=True)
    if offset == 0:
        assert key.check(offset, count, on_curve=on_curve, subgroup=subgroup) == (bad, first)      # the same without the bytes
    return bad, first, [int(v) for v in flags]
