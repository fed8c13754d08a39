"""Pure-Python restatement of sample_generators over the short Weierstrass curves (ipa_pc/mod.rs:302-325, hyrax/mod.rs:119-168) and of
InnerProductArgPC::setup / trim (:344-400) and HyraxPC::setup above it, for the tests of the device path (csrc/sw_setup.hpp,
abi_setup.hip, poly_commit_amd/setup.py): D = Blake2s256 from hashlib, short_weierstrass::Affine::from_random_bytes, the cofactor, all
over Python integers.  The curve numbers are those of oracle/pyref.py and tests/harness/ref377.py (read through ref377's private copy,
which holds all four curves); nothing is taken from the code under test.

from_random_bytes is restated from the published behaviour of ark-ec / ark-ff 0.5 and, like harness/te_setup.py's, NOT confirmed
against the crates:
  Fp::from_random_bytes_with_flags::<SWFlags> copies the 32 bytes into a buffer of ceil((bits + 2) / 8) bytes; the two flag bits are
  the top bits of the buffer's last byte
    BLS12-381, BLS12-377   48 bytes: the flags are clear, x is the 256-bit integer (always < p)
    Pallas                 33 bytes: the flags are clear, x = v mod 2^255, None at x >= p
    BN254                  32 bytes: the flags are bits 7 and 6 of byte 31, x = v mod 2^254, None at x >= p
  flags: 0x80 YIsNegative, 0x40 PointAtInfinity, both: None; PointAtInfinity is the identity at x = 0 and None otherwise
  y^2 = x^3 + b: None at a non-square, 0 is a square with root 0; the flag names the root (pick_root, the one place that decides it)
"""
import functools
import hashlib
import math

from harness import ref377

R = ref377.R
CURVES = ("bls12_381", "bn254", "pallas", "bls12_377")
CURVE_ID = {c: i for i, c in enumerate(CURVES)}                       # pc_curve
IPA_NAME, HYRAX_NAME = b"PC-DL-2020", b"Hyrax protocol"
ACCEPT, RANGE, NON_SQUARE, FLAGS = "accept", "x >= p", "non-square", "flags"
MAX_DIGESTS = 256


def field(curve):
    """-> (p, bits, 32-bit words of an element)"""
    f = R.FIELDS[R.CURVES[curve]["fq"]]
    return f["p"], f["p"].bit_length(), 2 * f["limbs64"]


def rhs(curve, x):
    p, _, b = R.curve_params(curve)
    return (x * x * x + b) % p


def is_square(curve, v):
    p = field(curve)[0]
    v %= p
    return v == 0 or pow(v, (p - 1) // 2, p) == 1


def sqrt(curve, v):
    """either root of a square (asserted); 0 for 0"""
    f = R.FIELDS[R.CURVES[curve]["fq"]]
    p = f["p"]
    v %= p
    if v == 0:
        return 0
    assert pow(v, (p - 1) // 2, p) == 1
    if p % 4 == 3:
        r = pow(v, (p + 1) // 4, p)
    else:
        s = R.two_adicity(p)
        t = (p - 1) >> s
        m, c, tt, r = s, pow(f["gen"], t, p), pow(v, t, p), pow(v, (t + 1) // 2, p)
        while tt != 1:
            i, x = 0, tt
            while x != 1:
                x, i = x * x % p, i + 1
            bb = pow(c, 1 << (m - i - 1), p)
            m, c = i, bb * bb % p
            tt, r = tt * c % p, r * bb % p
    assert r * r % p == v
    return r


def pick_root(p, y, y_is_negative):
    """THE mapping from SWFlags to a root, restated and NOT confirmed against ark-ec: the root that the project's compressed
    deserialisation takes for the same flag (oracle/pyref.py ser_point_compressed, pinned by BN254's (1, 2)): YIsPositive (no flag)
    is the root with y <= -y as canonical integers, YIsNegative the other.  y: either root."""
    lo, hi = min(y, (p - y) % p), max(y, (p - y) % p)
    return hi if y_is_negative else lo


def try_bytes(curve, digest):
    """Affine::from_random_bytes on 32 bytes -> (outcome, point); the point is None unless accepted, and R.INF (also None) for the
    identity BN254's flags can ask for: `outcome` tells the two apart"""
    p, bits, _ = field(curve)
    v = int.from_bytes(digest[:32], "little")
    neg = inf = 0
    if (bits + 2 + 7) // 8 <= 32:
        neg, inf = (v >> 255) & 1, (v >> 254) & 1
    x = v & ((1 << bits) - 1) if bits < 256 else v
    if x >= p:
        return RANGE, None
    if neg and inf:
        return FLAGS, None
    if inf:
        return (ACCEPT, R.INF) if x == 0 else (FLAGS, None)
    n = rhs(curve, x)
    if not is_square(curve, n):
        return NON_SQUARE, None
    return ACCEPT, (x, pick_root(p, sqrt(curve, n), bool(neg)))


@functools.lru_cache(None)
def cofactor(curve):
    """#E(Fq) / r: the one multiple of r in Hasse's interval around p + 1"""
    p, r, _ = R.curve_params(curve)
    sq = 2 * (math.isqrt(p) + 1)                                      # >= 2 sqrt(p)
    lo, hi = -(-(p + 1 - sq) // r), (p + 1 + sq) // r
    assert lo == hi
    return lo


def mul(curve, k, P):
    """k * P for an affine point (or R.INF), in Jacobian coordinates with one inversion: the cofactor and subgroup checks of a
    thousand points in a second, where R.ec_mul inverts at every step"""
    if P is R.INF or k == 0:
        return R.INF
    p = field(curve)[0]
    x, y = P
    X, Y, Z = x, y, 1
    for bit in bin(k)[3:]:
        if Z:                                                         # doubling, a = 0
            if Y == 0:
                X, Y, Z = 1, 1, 0
            else:
                A, B = X * X % p, Y * Y % p
                C = B * B % p
                D = 2 * ((X + B) * (X + B) - A - C) % p
                E = 3 * A % p
                X3 = (E * E - 2 * D) % p
                X, Y, Z = X3, (E * (D - X3) - 8 * C) % p, 2 * Y * Z % p
        if bit == "1":
            if not Z:
                X, Y, Z = x, y, 1
            else:                                                     # mixed addition
                ZZ = Z * Z % p
                U2, S2 = x * ZZ % p, y * Z * ZZ % p
                H, rr = (U2 - X) % p, (S2 - Y) % p
                if H == 0:
                    if rr == 0:                                       # the sum so far IS P (small torsion only): the plain ladder
                        return R.ec_mul(curve, k, P)
                    X, Y, Z = 1, 1, 0
                else:
                    HH = H * H % p
                    HHH, V = H * HH % p, X * HH % p
                    X3 = (rr * rr - HHH - 2 * V) % p
                    X, Y, Z = X3, (rr * (V - X3) - Y * HHH) % p, Z * H % p
    return to_affine(curve, (X, Y, Z))


def to_affine(curve, J):
    p = field(curve)[0]
    X, Y, Z = J
    if not Z:
        return R.INF
    zi = pow(Z, -1, p)
    return (X * zi * zi % p, Y * zi * zi % p * zi % p)


def digest(name, i, j=None):
    return hashlib.blake2s(name + i.to_bytes(8, "little") + (b"" if j is None else j.to_bytes(8, "little"))).digest()


@functools.lru_cache(None)
def trace(curve, name, i):
    """-> (the point before the cofactor, the accepted digest, the outcome of every digest in order)"""
    h = digest(name, i)
    why, g = try_bytes(curve, h)
    reasons, j = [why], 0
    while why != ACCEPT:
        assert len(reasons) < MAX_DIGESTS
        h = digest(name, i, j)
        why, g = try_bytes(curve, h)
        reasons.append(why)
        j += 1
    return g, h, tuple(reasons)


def digest_count(curve, name, i):
    return len(trace(curve, name, i)[2])


@functools.lru_cache(None)
def generator(curve, name, i):
    """generator i of sample_generators: (cofactor * g, the number of digests consumed); computed once per (curve, name, i)"""
    g, _, reasons = trace(curve, name, i)
    return mul(curve, cofactor(curve), g), len(reasons)


def generators(curve, name, first, count):
    """-> (points, digest counts) of the indices [first, first + count)"""
    out = [generator(curve, name, first + k) for k in range(count)]
    return [q for q, _ in out], [c for _, c in out]


def pow2_at_least(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def ipa_setup(curve, max_degree, name=IPA_NAME):
    """InnerProductArgPC::setup: max_degree + 1 rounded up to a power of two; the reference pops h first, so h is the last generator"""
    max_degree = pow2_at_least(max_degree + 1) - 1
    gens, _ = generators(curve, name, 0, max_degree + 3)
    return dict(comm_key=gens[:max_degree + 1], s=gens[max_degree + 1], h=gens[max_degree + 2], max_degree=max_degree)


def ipa_trim(pp, supported_degree):
    supported_degree = pow2_at_least(supported_degree + 1) - 1
    if supported_degree > pp["max_degree"]:
        raise ValueError("TrimmingDegreeTooLarge")
    return dict(comm_key=pp["comm_key"][:supported_degree + 1], s=pp["s"], h=pp["h"], supported_degree=supported_degree, max_degree=pp["max_degree"])


def hyrax_setup(curve, num_vars):
    """HyraxPC::setup (hyrax/mod.rs:119-168): 2^(n/2) + 1 points under b"Hyrax protocol", the last is h"""
    if num_vars is None or num_vars % 2 == 1:
        raise ValueError("InvalidNumberOfVariables")
    dim = 1 << (num_vars // 2)
    gens, _ = generators(curve, HYRAX_NAME, 0, dim + 1)
    return dict(com_key=gens[:dim], h=gens[dim])


# ---- integers <-> the ABI's Montgomery words -----------------------------------------------------------------------------------------

def mont(curve, v):
    p, _, n = field(curve)
    return v * (1 << (32 * n)) % p


def unmont(curve, v):
    p, _, n = field(curve)
    return v * pow(1 << (32 * n), -1, p) % p


def point_words(curve, P):
    """an affine point (or R.INF) -> its 2 n little-endian 32-bit words x || y in Montgomery form; the identity is all zero"""
    n = field(curve)[2]
    if P is R.INF:
        return [0] * (2 * n)
    return [(mont(curve, c) >> (32 * k)) & 0xffffffff for c in P for k in range(n)]


def point_of_words(curve, words):
    n = field(curve)[2]
    w = [int(x) for x in words]
    assert len(w) == 2 * n
    if not any(w):
        return R.INF
    x, y = (sum(v << (32 * k) for k, v in enumerate(w[h * n:(h + 1) * n])) for h in (0, 1))
    p = field(curve)[0]
    assert x < p and y < p, "a coordinate left [0, p)"
    return (unmont(curve, x), unmont(curve, y))
