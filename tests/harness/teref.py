"""Pure-Python restatement of the twisted Edwards curve ed_on_bls12_381 (JubJub) for the tests of the device path (csrc/te.hpp,
abi_te.hip): the complete affine law over Python integers, scalar multiplication, a small Pippenger, a fixed-base helper for making
keys, and the byte forms of the C ABI.  Nothing here uses r P = O: every product is exact integer arithmetic on the point it is
given, as ark-ec's msm_bigint is, so bases with a low-order component have well-defined expected values.

A point is an (x, y) tuple of integers below Q; the identity is (0, 1).  ZERO = (0, 0) is the all-zero key entry, which is not a curve
point and counts as the identity wherever it is an input."""
import numpy as np

Q = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001      # the coordinate field: BLS12-381's Fr
R = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7      # the prime subgroup order (252 bits)
COFACTOR = 8
A = Q - 1
D = (-10240 * pow(10241, -1, Q)) % Q
D2 = 2 * D % Q
GEN = (8076246640662884909881801758704306714034609987455869804520522091855516602923,
       13262374693698910701929044844600465831413122818447359594527400194675274060458)
IDENT = (0, 1)
ZERO = (0, 0)
MONT_Q = (1 << 256) % Q
MONT_R = (1 << 256) % R
FQ_BYTES = 32
POINT_BYTES = 64


def on_curve(p):
    x, y = p
    return (A * x * x + y * y - 1 - D * x * x % Q * y * y) % Q == 0


def _pt(p):
    return IDENT if p == ZERO else p


def add(p, q):
    """the complete affine law: no exceptional inputs (a is a square, d is not)"""
    (x1, y1), (x2, y2) = _pt(p), _pt(q)
    t = D * x1 * x2 % Q * y1 * y2 % Q
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, Q) % Q, (y1 * y2 - A * x1 * x2) * pow(1 - t, -1, Q) % Q)


def neg(p):
    x, y = _pt(p)
    return ((Q - x) % Q, y)


# extended coordinates (X, Y, Z, T) with a = -1 over Python integers: the fast path of mul / msm / FixedBase
_E_ID = (0, 1, 1, 0)


def _e_from(p):
    x, y = _pt(p)
    return (x, y, 1, x * y % Q)


def _e_add(p, q):
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    a = (Y1 - X1) * (Y2 - X2) % Q
    b = (Y1 + X1) * (Y2 + X2) % Q
    c = T1 * D2 % Q * T2 % Q
    d = 2 * Z1 * Z2 % Q
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % Q, g * h % Q, f * g % Q, e * h % Q)


def _e_dbl(p):
    X1, Y1, Z1, _ = p
    a, b, c = X1 * X1 % Q, Y1 * Y1 % Q, 2 * Z1 * Z1 % Q
    d = -a
    e = ((X1 + Y1) * (X1 + Y1) - a - b) % Q
    g = d + b
    f, h = g - c, d - b
    return (e * f % Q, g * h % Q, f * g % Q, e * h % Q)


def _e_affine(p):
    X, Y, Z, _ = p
    zi = pow(Z, -1, Q)
    return (X * zi % Q, Y * zi % Q)


def _e_affine_batch(ps):
    pre, run = [], 1
    for p in ps:
        pre.append(run)
        run = run * p[2] % Q
    inv = pow(run, -1, Q)
    out = [None] * len(ps)
    for i in range(len(ps) - 1, -1, -1):
        zi = inv * pre[i] % Q
        inv = inv * ps[i][2] % Q
        out[i] = (ps[i][0] * zi % Q, ps[i][1] * zi % Q)
    return out


def _e_mul(k, p):
    acc, base = _E_ID, _e_from(p)
    for bit in bin(k)[2:] if k else "":
        acc = _e_dbl(acc)
        if bit == "1":
            acc = _e_add(acc, base)
    return acc


def mul(k, p):
    """k * p for the non-negative INTEGER k (not reduced modulo r: p may lie outside the prime-order subgroup)"""
    assert k >= 0
    return _e_affine(_e_mul(k, p))


def msm(bases, scalars, c=None):
    """sum scalars[i] * bases[i] over min(len) pairs, integer-exact: a small Pippenger with unsigned radix-2^c digits"""
    n = min(len(bases), len(scalars))
    if n == 0:
        return IDENT
    ks = [int(k) for k in scalars[:n]]
    ext = [_e_from(b) for b in bases[:n]]
    bits = max(1, max(ks).bit_length())
    if c is None:
        c = 1 if n < 4 else max(2, min(12, n.bit_length() - 2))
    acc = _E_ID
    for w in range((bits + c - 1) // c - 1, -1, -1):
        for _ in range(c):
            acc = _e_dbl(acc)
        buckets = {}
        for k, p in zip(ks, ext):
            dgt = (k >> (w * c)) & ((1 << c) - 1)
            if dgt:
                buckets[dgt] = _e_add(buckets[dgt], p) if dgt in buckets else p
        run, tot = _E_ID, _E_ID
        for dgt in range((1 << c) - 1, 0, -1):
            if dgt in buckets:
                run = _e_add(run, buckets[dgt])
            if run is not _E_ID:
                tot = _e_add(tot, run)
        acc = _e_add(acc, tot)
    return _e_affine(acc)


class FixedBase:
    """k * B for many k: 8-bit windows of B, one batch normalisation"""

    def __init__(self, B, bits=256):
        self.tbl = []
        cur = _e_from(B)
        for _ in range((bits + 7) // 8):
            row, acc = [_E_ID], _E_ID
            for _ in range(255):
                acc = _e_add(acc, cur)
                row.append(acc)
            self.tbl.append(row)
            cur = _e_add(acc, cur)

    def mul_many(self, ks):
        out = []
        for k in ks:
            acc, w = _E_ID, 0
            while k:
                if k & 255:
                    acc = _e_add(acc, self.tbl[w][k & 255])
                k >>= 8
                w += 1
            out.append(acc)
        return _e_affine_batch(out)


_FB = {}


def fixed_base(B):
    if B not in _FB:
        _FB[B] = FixedBase(B)
    return _FB[B]


def _sqrt(v):
    """Tonelli-Shanks in Fq"""
    v %= Q
    assert pow(v, (Q - 1) // 2, Q) == 1
    s, t = 0, Q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (Q - 1) // 2, Q) != Q - 1:
        z += 1
    m, cc, tt, r = s, pow(z, t, Q), pow(v, t, Q), pow(v, (t + 1) // 2, Q)
    while tt != 1:
        i, x = 0, tt
        while x != 1:
            x, i = x * x % Q, i + 1
        b = pow(cc, 1 << (m - i - 1), Q)
        m, cc = i, b * b % Q
        tt, r = tt * cc % Q, r * b % Q
    return r


def point_with_y(y):
    """a curve point with this y (the smaller of the two x)"""
    x = _sqrt((1 - y * y) * pow(A - D * y * y, -1, Q))
    return (min(x, Q - x), y)


# the low-order points: legal MSM and fold input
T2 = (0, Q - 1)                                       # order 2
T4 = point_with_y(0)                                  # order 4
T8 = mul(R, point_with_y(11))                         # order 8

# facts the device code relies on, asserted at import
assert pow(A, (Q - 1) // 2, Q) == 1 and pow(D, (Q - 1) // 2, Q) == Q - 1, "a square, d non-square: the law is complete"
assert on_curve(GEN) and mul(R, GEN) == IDENT and GEN != IDENT
assert on_curve(T2) and mul(2, T2) == IDENT
assert on_curve(T4) and mul(2, T4) == T2
assert on_curve(T8) and mul(4, T8) == T2 and mul(8, T8) == IDENT and mul(2, T8) in (T4, neg(T4))
assert add(GEN, neg(GEN)) == IDENT and add(GEN, GEN) == mul(2, GEN) and add(IDENT, T8) == T8
assert (R - 1) % 4 == 2, "2-adicity 1"


# ---- the byte forms of the C ABI: Montgomery residues, little-endian --------------------------------------------------------
def point_bytes(p):
    x, y = p
    return (x * MONT_Q % Q).to_bytes(32, "little") + (y * MONT_Q % Q).to_bytes(32, "little")


def points_array(pts):
    return np.frombuffer(b"".join(point_bytes(p) for p in pts), dtype=np.uint8).reshape(len(pts), POINT_BYTES).copy()


def point_from_bytes(b):
    ri = pow(MONT_Q, -1, Q)
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")
    assert x < Q and y < Q, "a coordinate left [0, q)"
    return (x * ri % Q, y * ri % Q)


IDENT_BYTES = point_bytes(IDENT)                      # (0, ONE): arkworks' Affine::zero()


def scalars_array(ks, mont):
    return np.frombuffer(b"".join(((k * MONT_R % R) if mont else k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(len(ks), 32).copy()


def resident_words(p):
    """the device's form of a base: x || y || 2 d x y (Montgomery), 24 words; ZERO stays all zero"""
    x, y = p
    td = D2 * x * y % Q
    return np.frombuffer(point_bytes(p) + (td * MONT_Q % Q).to_bytes(32, "little"), dtype=np.uint32).copy()


def fold(key, u):
    """one key fold of InnerProductArgPC::open: out[i] = key[i] + u * key[half + i] (u the integer)"""
    half = len(key) // 2
    return [add(key[i], mul(u, key[half + i])) for i in range(half)]
