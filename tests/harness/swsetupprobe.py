"""Case tables and checks of the short Weierstrass sample_generators probe (tests/hip/probe_sw_setup.hip): shared by
tests/test_sw_setup_cpu.py, which runs them through the host build of the probe, and tests/test_sw_primitives_gpu.py, which runs them on
the device and also compares every output word with the host build's -- the way tests/harness/tesetupprobe.py serves ed_on_bls12_381.

The references are tests/harness/sw_setup.py (from_random_bytes, the cofactor and sample_generators over Python integers), hashlib's
blake2s and Python integers; nothing is taken from the code under test.  Every check takes `probe` (the library under test) and `host`
(the host build; the same object in the CPU suite) and returns its lane count: the tests assert the exact number."""
import ctypes as C
import functools
import random

import numpy as np

from harness import ref377
from harness import sw_setup as S

R = S.R
CURVES = S.CURVES
TRY_CODE = {S.ACCEPT: 0, S.RANGE: 1, S.NON_SQUARE: 2, S.FLAGS: 3}      # pc::SW_TRY_* (csrc/sw_setup.hpp)
TWO_ADIC = ("pallas", "bls12_377")                                     # Tonelli-Shanks; the other two take n^((p + 1) / 4)


def P():
    return ref377.probe()


def host_probe():
    return P().host_probe()


def device_probe():
    return P().device_probe()


def twin(name, probe_, host, run):
    """run(library) -> output words; on the device the host build's words must be the same"""
    out = run(probe_)
    if host is not probe_:
        P().same_words(name, out, run(host))
    return out


def mont_words(curve, vals):
    n = S.field(curve)[2]
    return P().pack([S.mont(curve, v) for v in vals], n)


def from_mont(curve, rows):
    p = S.field(curve)[0]
    vals = P().unpack(rows)
    assert all(v < p for v in vals), "a residue left [0, p)"
    return [S.unmont(curve, v) for v in vals]


def curve_point(curve, rnd):
    """a seeded point of the curve, of full order with overwhelming probability (not in the subgroup where the cofactor is not 1)"""
    p = S.field(curve)[0]
    while True:
        x = rnd.randrange(p)
        n = S.rhs(curve, x)
        if n and S.is_square(curve, n):
            return (x, S.sqrt(curve, n))


# ---- the square root ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def sqrt_cases(curve):
    """0, 1, 4, p - 1, the field's non-residue g, the generator's x^3 + b; for the two-adic fields c = g^t (a non-square of maximal
    order 2^S), c^2 (a square whose n^t has order 2^(S-1): the longest Tonelli run) and c^(2^(S-1)) = -1; 64 seeded squares and 64
    seeded non-squares"""
    f = R.FIELDS[R.CURVES[curve]["fq"]]
    p, g = f["p"], f["gen"]
    assert not S.is_square(curve, g)
    vals = [0, 1, 4, p - 1, g, S.rhs(curve, R.CURVES[curve]["gx"])]
    if curve in TWO_ADIC:
        s = R.two_adicity(p)
        c = pow(g, (p - 1) >> s, p)
        assert pow(c, 1 << (s - 1), p) == p - 1
        vals += [c, c * c % p, pow(c, 1 << (s - 1), p)]
        assert not S.is_square(curve, c) and S.is_square(curve, c * c % p)
    rnd = random.Random(4646 + S.CURVE_ID[curve])
    sq = [pow(rnd.randrange(1, p), 2, p) for _ in range(64)]
    vals += sq + [g * v % p for v in sq[::-1]]
    return tuple(vals)


def sqrt_lanes(curve):
    return 6 + (3 if curve in TWO_ADIC else 0) + 128


def check_sqrt(probe_, host, curve):
    p, _, n = S.field(curve)
    vals = sqrt_cases(curve)
    inp = mont_words(curve, vals)

    def run(pr):
        out = np.zeros((len(vals), n + 1), dtype=np.uint32)
        pr.call("pc_probe_sw_setup_sqrt", C.c_int(S.CURVE_ID[curve]), C.c_size_t(len(vals)), P().p32(inp), P().p32(out))
        return out
    out = twin("sw_setup sqrt " + curve, probe_, host, run)
    roots = from_mont(curve, out[:, :n])
    for i, (v, r) in enumerate(zip(vals, roots)):
        want = 1 if S.is_square(curve, v) else 0
        assert out[i, n] == want, "%s sqrt lane %d: %x is %sa square" % (curve, i, v, "" if want else "not ")
        assert r * r % p == (v if want else 0), "%s sqrt lane %d: the root of %x squares to something else" % (curve, i, v)
    assert [int(f) for f in out[-128:, n]] == [1] * 64 + [0] * 64
    return len(vals)


# ---- from_random_bytes -------------------------------------------------------------------------------------------------------------

def le32(v):
    return v.to_bytes(32, "little")


@functools.lru_cache(None)
def straddlers(curve):
    """(x whose square root, as n^((p+1)/4) or Tonelli-Shanks returns it, is the smaller of the pair; x where it is the larger): the
    flag's root is then once the computed root and once its negative.  Both below 2^254 with room for the flag bits."""
    p = S.field(curve)[0]
    low = high = None
    x = 2
    while low is None or high is None:
        n = S.rhs(curve, x)
        if n and S.is_square(curve, n):
            r = S.sqrt(curve, n)
            if r <= (p - 1) // 2 and low is None:
                low = x
            if r > (p - 1) // 2 and high is None:
                high = x
        x += 1
    return low, high


@functools.lru_cache(None)
def try_cases(curve):
    """the crafted digests of the issue, then every digest the indices 0..15 of PC-DL-2020 consume"""
    p, bits, _ = S.field(curve)
    cases = [bytes(32), bytes(31) + b"\x40", b"\xff" * 32]
    if bits < 256:                                        # x = p - 1, p, p + 1 under the field's mask
        cases += [le32(p - 1), le32(p), le32(p + 1)]
    low, high = straddlers(curve)
    for x in (low, high):                                 # the four flag combinations (flags only where the buffer ends inside the digest)
        cases += [le32(x | (f << 254)) for f in range(4)]
    cases.append(le32(low | (1 << 255)))                  # bit 255: Pallas masks it away, BN254 reads YIsNegative, the BLS curves a larger x
    for i in range(16):
        k = S.digest_count(curve, S.IPA_NAME, i)
        cases += [S.digest(S.IPA_NAME, i)] + [S.digest(S.IPA_NAME, i, j) for j in range(k - 1)]
    return tuple(cases)


def try_lanes(curve):
    return 3 + (3 if S.field(curve)[1] < 256 else 0) + 8 + 1 + sum(S.digest_count(curve, S.IPA_NAME, i) for i in range(16))


def check_try(probe_, host, curve):
    n = S.field(curve)[2]
    cases = try_cases(curve)
    inp = np.frombuffer(b"".join(cases), dtype=np.uint32).reshape(len(cases), 8).copy()

    def run(pr):
        out = np.zeros((len(cases), 1 + 2 * n), dtype=np.uint32)
        pr.call("pc_probe_sw_setup_try", C.c_int(S.CURVE_ID[curve]), C.c_size_t(len(cases)), P().p32(inp), P().p32(out))
        return out
    out = twin("sw_setup from_random_bytes " + curve, probe_, host, run)
    seen = set()
    for k, d in enumerate(cases):
        why, pt = S.try_bytes(curve, d)
        seen.add(why)
        assert out[k, 0] == TRY_CODE[why], "%s from_random_bytes lane %d (%s): outcome %d, want %s" % (curve, k, d.hex(), out[k, 0], why)
        assert [int(w) for w in out[k, 1:]] == (S.point_words(curve, pt) if why == S.ACCEPT else [0] * (2 * n)), \
            "%s from_random_bytes lane %d (%s): another point" % (curve, k, d.hex())
    # every outcome the curve can produce was produced
    want = {S.ACCEPT, S.NON_SQUARE} | ({S.RANGE} if S.field(curve)[1] < 256 else set()) | ({S.FLAGS} if curve == "bn254" else set())
    assert seen == want, (curve, seen)
    return len(cases)


# ---- the cofactor ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def cofactor_cases(curve):
    """the identity, the generator, eight seeded points of the curve and, where the cofactor is not 1, r * P for four of them: points
    of the cofactor torsion, whose image must be the identity"""
    r = R.curve_params(curve)[1]
    rnd = random.Random(8080 + S.CURVE_ID[curve])
    pts = [curve_point(curve, rnd) for _ in range(8)]
    cases = [R.INF, R.generator(curve)] + pts
    if S.cofactor(curve) != 1:
        torsion = [S.mul(curve, r, q) for q in pts[:4]]
        assert all(t is not R.INF and R.on_curve(curve, t) for t in torsion)
        cases += torsion
    return tuple(cases)


def cofactor_lanes(curve):
    return 10 + (4 if S.cofactor(curve) != 1 else 0)


def check_xyzz(name, curve, row, want):
    """a row of stored XYZZ words stands for `want`: canonical coordinates, ZZ = 0 exactly for the identity, ZZ^3 = ZZZ^2"""
    p, _, n = S.field(curve)
    X, Y, ZZ, ZZZ = from_mont(curve, row.reshape(4, n))
    if want is R.INF:
        assert ZZ == 0, "%s: the identity has ZZ != 0" % name
        return
    assert ZZ != 0 and pow(ZZ, 3, p) == ZZZ * ZZZ % p, "%s: ZZ^3 != ZZZ^2" % name
    got = (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)
    assert got == want, "%s: the stored words are the point %s, want %s" % (name, got, want)


def check_cofactor(probe_, host, curve):
    n = S.field(curve)[2]
    cases = cofactor_cases(curve)
    h = S.cofactor(curve)
    inp = np.array([S.point_words(curve, q) for q in cases], dtype=np.uint32)

    def run(pr):
        out = np.zeros((len(cases), 4 * n), dtype=np.uint32)
        pr.call("pc_probe_sw_setup_cofactor", C.c_int(S.CURVE_ID[curve]), C.c_size_t(len(cases)), P().p32(inp), P().p32(out))
        return out
    out = twin("sw_setup cofactor " + curve, probe_, host, run)
    wants = [S.mul(curve, h, q) for q in cases]
    for k, want in enumerate(wants):
        check_xyzz("%s cofactor lane %d" % (curve, k), curve, out[k], want)
    assert wants[0] is R.INF and wants[1] == (R.generator(curve) if h == 1 else R.ec_mul(curve, h, R.generator(curve)))
    assert all(w is R.INF for w in wants[10:]) and all(w is not R.INF for w in wants[1:10])
    return len(cases)


# ---- the per-index body --------------------------------------------------------------------------------------------------------------

SAMPLE_RANGES = ((0, 64), ((1 << 32) - 1, 2))      # indices 0..63, the two sides of le64's word edge


def run_sample(pr, curve, name, first, count):
    n = S.field(curve)[2]
    out, dg, failed = np.zeros((count, 2 * n), dtype=np.uint32), np.zeros(count, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    pr.call("pc_probe_sw_setup_sample", C.c_int(S.CURVE_ID[curve]), name, C.c_size_t(len(name)), C.c_uint64(first), C.c_size_t(count),
            P().p32(out), P().p32(dg), P().p32(failed))
    return np.concatenate([out.reshape(-1), dg, failed])


def check_sample(probe_, host, curve):
    """SwSampleBody: the point BEFORE the cofactor and the digest count of every index"""
    n = S.field(curve)[2]
    lanes = 0
    for first, count in SAMPLE_RANGES:
        out = twin("sw_setup sample " + curve, probe_, host, lambda pr: run_sample(pr, curve, S.IPA_NAME, first, count))
        pts, dg, failed = out[:count * 2 * n].reshape(count, 2 * n), out[count * 2 * n:count * 2 * n + count], out[-1]
        assert failed == 0
        for k in range(count):
            g, _, reasons = S.trace(curve, S.IPA_NAME, first + k)
            assert int(dg[k]) == len(reasons), "%s index %d: %d digests, want %d" % (curve, first + k, dg[k], len(reasons))
            assert [int(w) for w in pts[k]] == S.point_words(curve, g), "%s index %d: another point" % (curve, first + k)
        lanes += count
    return lanes
