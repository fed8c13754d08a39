"""Pure-Python reference for G2 of BLS12-381 and for MultilinearPC (poly-commit/src/multilinear_pc/mod.rs): test infrastructure only.

Fq2 = Fq[u]/(u^2 + 1) as pairs of Python ints, the twist E': y^2 = x^3 + 4(1 + u) in Jacobian coordinates (affine results are
canonical, so the coordinate system is free), scalar multiplication, a small Pippenger, a fixed-base window table, and a literal
restatement of MultilinearPC's setup / commit / open (mod.rs:28-168, including the `x >> 1` of :158-160).  The moduli come from
oracle/pyref.py; nothing here depends on the standard G2 generator: `generator()` derives its own point of order r.

A point is None (infinity) or ((x0, x1), (y0, y1)).  G1 points are handled by the same code with x1 = y1 = 0: for a = 0 the group
law does not see the constant b, and Fq is a subfield of Fq2.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402

P = pyref.FIELDS["bls12_381_fq"]["p"]
R = pyref.FIELDS["bls12_381_fr"]["p"]
BLS_X = -0xd201000000010000          # the curve parameter
B2 = (4, 4)                          # b' = 4 (1 + u)
MONT_Q = (1 << 384) % P
MONT_R = (1 << 256) % R
INF = None

# ---- Fq2 --------------------------------------------------------------------------------------


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return ((a[0] + a[1]) * (a[0] - a[1]) % P, 2 * a[0] * a[1] % P)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P) if (a[0] or a[1]) else 0
    return (a[0] * n % P, (-a[1]) * n % P)


def f2_mul_add_mul(a, b, c, d):
    return f2_add(f2_mul(a, b), f2_mul(c, d))


def _fq_sqrt(a):
    """p = 3 (mod 4)"""
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def f2_sqrt(a):
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = _fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = _fq_sqrt((-a0) % P)
        return (0, s)
    alpha = _fq_sqrt((a0 * a0 + a1 * a1) % P)
    if alpha is None:
        return None
    inv2 = pow(2, -1, P)
    for al in (alpha, (-alpha) % P):
        x0 = _fq_sqrt((a0 + al) * inv2 % P)
        if x0 is not None and x0 != 0:
            x1 = a1 * pow(2 * x0, -1, P) % P
            if f2_sqr((x0, x1)) == (a0, a1):
                return (x0, x1)
    return None


# ---- the group law (Jacobian, a = 0), over Fq2 -------------------------------------------------

def on_twist(Pt):
    if Pt is INF:
        return True
    x, y = Pt
    return f2_sqr(y) == f2_add(f2_mul(f2_sqr(x), x), B2)


def neg(Pt):
    return INF if Pt is INF else (Pt[0], f2_neg(Pt[1]))


_J_INF = ((1, 0), (1, 0), (0, 0))


def _j_is_inf(J):
    return J[2] == (0, 0)


def _j_from(Pt):
    return _J_INF if Pt is INF else (Pt[0], Pt[1], (1, 0))


def _j_dbl(J):
    X, Y, Z = J
    if Z == (0, 0) or Y == (0, 0):
        return _J_INF
    A = f2_sqr(X); B = f2_sqr(Y); C = f2_sqr(B)
    t = f2_sub(f2_sub(f2_sqr(f2_add(X, B)), A), C)
    D = f2_add(t, t)
    E = f2_add(f2_add(A, A), A)
    F = f2_sqr(E)
    X3 = f2_sub(F, f2_add(D, D))
    C8 = f2_add(C, C); C8 = f2_add(C8, C8); C8 = f2_add(C8, C8)
    Y3 = f2_sub(f2_mul(E, f2_sub(D, X3)), C8)
    YZ = f2_mul(Y, Z)
    return (X3, Y3, f2_add(YZ, YZ))


def _j_add(J1, J2):
    if _j_is_inf(J1):
        return J2
    if _j_is_inf(J2):
        return J1
    X1, Y1, Z1 = J1
    X2, Y2, Z2 = J2
    Z1Z1 = f2_sqr(Z1); Z2Z2 = f2_sqr(Z2)
    U1 = f2_mul(X1, Z2Z2); U2 = f2_mul(X2, Z1Z1)
    S1 = f2_mul(f2_mul(Y1, Z2), Z2Z2); S2 = f2_mul(f2_mul(Y2, Z1), Z1Z1)
    H = f2_sub(U2, U1); r = f2_sub(S2, S1)
    if H == (0, 0):
        return _j_dbl(J1) if r == (0, 0) else _J_INF
    HH = f2_sqr(H); HHH = f2_mul(H, HH); V = f2_mul(U1, HH)
    X3 = f2_sub(f2_sub(f2_sqr(r), HHH), f2_add(V, V))
    Y3 = f2_sub(f2_mul(r, f2_sub(V, X3)), f2_mul(S1, HHH))
    return (X3, Y3, f2_mul(f2_mul(Z1, Z2), H))


def _j_affine(J):
    if _j_is_inf(J):
        return INF
    zi = f2_inv(J[2]); zi2 = f2_sqr(zi)
    return (f2_mul(J[0], zi2), f2_mul(f2_mul(J[1], zi2), zi))


def _j_affine_batch(Js):
    """Montgomery's trick: one inversion for all"""
    pre, run = [], (1, 0)
    for J in Js:
        pre.append(run)
        if not _j_is_inf(J):
            run = f2_mul(run, J[2])
    inv = f2_inv(run)
    out = [INF] * len(Js)
    for i in range(len(Js) - 1, -1, -1):
        J = Js[i]
        if _j_is_inf(J):
            continue
        zi = f2_mul(inv, pre[i]); inv = f2_mul(inv, J[2])
        zi2 = f2_sqr(zi)
        out[i] = (f2_mul(J[0], zi2), f2_mul(f2_mul(J[1], zi2), zi))
    return out


def add(A, B):
    return _j_affine(_j_add(_j_from(A), _j_from(B)))


def _j_mul(k, Pt):
    acc, J = _J_INF, _j_from(Pt)
    for bit in bin(k)[2:]:
        acc = _j_dbl(acc)
        if bit == "1":
            acc = _j_add(acc, J)
    return acc


def mul(k, Pt, mod_r=True):
    """k * Pt (k reduced mod r unless mod_r is False: cofactor clearing, order checks)"""
    if mod_r:
        k %= R
    return _j_affine(_j_mul(k, Pt)) if k else INF


def msm(bases, scalars, c=None):
    """sum k_i P_i over min(len) pairs (msm_bigint's truncation), by a small Pippenger"""
    n = min(len(bases), len(scalars))
    if n == 0:
        return INF
    ks = [int(k) % R for k in scalars[:n]]
    if n < 8:
        acc = _J_INF
        for Pt, k in zip(bases, ks):
            if k and Pt is not INF:
                acc = _j_add(acc, _j_mul(k, Pt))
        return _j_affine(acc)
    if c is None:
        c = max(2, min(12, n.bit_length() - 2))
    Js = [_j_from(Pt) for Pt in bases[:n]]
    W = (255 + c - 1) // c
    total = _J_INF
    for w in range(W - 1, -1, -1):
        for _ in range(c):
            total = _j_dbl(total)
        buckets = {}
        for J, k in zip(Js, ks):
            d = (k >> (w * c)) & ((1 << c) - 1)
            if d and not _j_is_inf(J):
                buckets[d] = _j_add(buckets[d], J) if d in buckets else J
        run, acc = _J_INF, _J_INF
        for d in range(max(buckets) if buckets else 0, 0, -1):
            if d in buckets:
                run = _j_add(run, buckets[d])
            acc = _j_add(acc, run)
        total = _j_add(total, acc)
    return _j_affine(total)


class FixedBase:
    """k * B for many k: 32 windows of 8 bits, table[w][d - 1] = d * 2^(8 w) * B (mixed-free Jacobian adds: 32 per product)"""

    def __init__(self, B):
        self.tbl = []
        cur = _j_from(B)
        for _ in range(32):
            row, acc = [], _J_INF
            for _d in range(255):
                acc = _j_add(acc, cur)
                row.append(acc)
            self.tbl.append(row)
            cur = _j_add(acc, cur)                       # 256 * cur
        flat = _j_affine_batch([J for row in self.tbl for J in row])
        self.tbl = [[_j_from(flat[w * 255 + d]) for d in range(255)] for w in range(32)]

    def mul_many(self, ks):
        out = []
        for k in ks:
            k %= R
            acc = _J_INF
            for w in range(32):
                d = (k >> (8 * w)) & 0xff
                if d:
                    acc = _j_add(acc, self.tbl[w][d - 1])
            out.append(acc)
        return _j_affine_batch(out)


_FB = {}


def fixed_base(B):
    if B not in _FB:
        _FB[B] = FixedBase(B)
    return _FB[B]


# ---- a generator of G2 of our own --------------------------------------------------------------

def _twist_orders():
    """candidate group orders of the sextic twists of E over Fq2, from the trace (t = x + 1 over Fq)"""
    q = P
    t1 = BLS_X + 1
    assert (q + 1 - t1) % R == 0                          # #E(Fq) is divisible by r
    t2 = t1 * t1 - 2 * q                                  # trace over Fq2
    f2sq = (4 * q * q - t2 * t2) // 3                     # t2^2 - 4 q^2 = -3 f^2
    import math
    f = math.isqrt(f2sq)
    assert f * f == f2sq
    return [q * q + 1 - (s1 * t2 + s2 * 3 * f) // 2 for s1 in (1, -1) for s2 in (1, -1)]


_GEN = None


def generator():
    """A point of order r on the twist: the first x = c + 0u, c = 1, 2, .. with x^3 + 4(1 + u) a square, times the G2 cofactor.
    The cofactor comes from the closed form in the curve parameter; if the result is not annihilated by r it is derived from the
    trace instead."""
    global _GEN
    if _GEN is not None:
        return _GEN
    x = BLS_X
    h2 = (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9
    cofactors = [h2] + [n // R for n in _twist_orders() if n % R == 0]
    c = 0
    while True:
        c += 1
        X = (c, 0)
        y = f2_sqrt(f2_add(f2_mul(f2_sqr(X), X), B2))
        if y is None:
            continue
        Q = (X, y)
        assert on_twist(Q)
        for h in cofactors:
            G = mul(h, Q, mod_r=False)
            if G is not INF and on_twist(G) and mul(R, G, mod_r=False) is INF:
                _GEN = G
                return G
        raise AssertionError("no cofactor candidate clears the twist point to order r")


def g1_generator():
    g = pyref.generator("bls12_381")
    return ((g[0], 0), (g[1], 0))


# ---- bytes: Montgomery residues, little-endian, as the device and arkworks hold them --------------

def point_bytes(Pt, g1=False):
    """192 bytes x.c0 || x.c1 || y.c0 || y.c1 (all zero: infinity); g1: 96 bytes x || y"""
    if Pt is INF:
        return bytes(96 if g1 else 192)
    vals = (Pt[0][0], Pt[1][0]) if g1 else (Pt[0][0], Pt[0][1], Pt[1][0], Pt[1][1])
    return b"".join((v * MONT_Q % P).to_bytes(48, "little") for v in vals)


def points_array(pts, g1=False):
    w = 96 if g1 else 192
    return np.frombuffer(b"".join(point_bytes(p, g1) for p in pts), dtype=np.uint8).reshape(len(pts), w).copy()


def point_from_bytes(b, g1=False):
    b = bytes(b)
    if not any(b):
        return INF
    rinv = pow(MONT_Q, -1, P)
    v = [int.from_bytes(b[48 * i:48 * i + 48], "little") * rinv % P for i in range(2 if g1 else 4)]
    return ((v[0], 0), (v[1], 0)) if g1 else ((v[0], v[1]), (v[2], v[3]))


def scalars_array(ks, mont):
    """n x 32 bytes: canonical residues (msm_bigint's argument) or Montgomery residues (Fr as it lies in memory)"""
    return np.frombuffer(b"".join(((k % R) * (MONT_R if mont else 1) % R).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(len(ks), 32).copy()


def scalars_from_array(a, mont):
    rinv = pow(MONT_R, -1, R)
    return [int.from_bytes(bytes(row), "little") * (rinv if mont else 1) % R for row in np.asarray(a, dtype=np.uint8).reshape(-1, 32)]


# ---- MultilinearPC, restated (multilinear_pc/mod.rs) -----------------------------------------------

def _eq_extension(t):
    """mod.rs:219-234"""
    dim = len(t)
    out = []
    for i in range(dim):
        poly = []
        for x in range(1 << dim):
            xi = (x >> i) & 1
            ti_xi = t[i] * xi % R
            poly.append((ti_xi + ti_xi - xi - t[i] + 1) % R)
        out.append(poly)
    return out


def _remove_dummy_variable(poly, pad):
    """mod.rs:204-214"""
    if pad == 0:
        return list(poly)
    nv = len(poly).bit_length() - 1 - pad
    return [poly[x << pad] for x in range(1 << nv)]


def ml_setup_with_trapdoor(nv, t, g=None, h=None):
    """mod.rs:28-86 with the trapdoor t (nv scalars) and the two generators given.  Returns a dict with powers_of_g / powers_of_h
    (lists of nv lists, level i of 2^(nv - i) points), g, h, t."""
    assert nv > 0 and len(t) == nv
    g = g1_generator() if g is None else g
    h = generator() if h is None else h
    eq = _eq_extension(t)
    eq_arr = []
    base = eq.pop()
    for i in range(nv - 1, -1, -1):
        eq_arr.insert(0, _remove_dummy_variable(base, i))
        if i != 0:
            m = eq.pop()
            base = [a * b % R for a, b in zip(base, m)]
    pp_powers = []
    for i in range(nv):
        pp_powers.extend(eq_arr[i][x] for x in range(1 << (nv - i)))
    pp_g = fixed_base(g).mul_many(pp_powers)
    pp_h = fixed_base(h).mul_many(pp_powers)
    powers_of_g, powers_of_h, start = [], [], 0
    for i in range(nv):
        size = 1 << (nv - i)
        powers_of_g.append(pp_g[start:start + size]); powers_of_h.append(pp_h[start:start + size])
        start += size
    return dict(nv=nv, g=g, h=h, t=list(t), powers_of_g=powers_of_g, powers_of_h=powers_of_h)


def ml_commit(ck, evals):
    """mod.rs:114-128"""
    return msm(ck["powers_of_g"][0], evals)


def ml_fold(r, z):
    """one round of mod.rs:153-157: (q, r_next)"""
    half = len(r) // 2
    q = [(r[2 * b + 1] - r[2 * b]) % R for b in range(half)]
    nxt = [(r[2 * b] * (1 - z) + r[2 * b + 1] * z) % R for b in range(half)]
    return q, nxt


def ml_open(ck, evals, point):
    """mod.rs:131-168, literally: round i multiplies ALL 2^(nv - i) points of powers_of_h[i] with scalars[x] = q[x >> 1]"""
    nv = ck["nv"]
    assert len(evals) == 1 << nv and len(point) == nv
    r = [e % R for e in evals]
    proofs = []
    for i in range(nv):
        k = nv - i
        q, r = ml_fold(r, point[i] % R)
        scalars = [q[x >> 1] for x in range(1 << k)]
        proofs.append(msm(ck["powers_of_h"][i], scalars))
    return proofs


def mle_eval(evals, point):
    r = [e % R for e in evals]
    for z in point:
        _, r = ml_fold(r, z % R)
    return r[0]


def ml_trapdoor_check(h, t, evals, point, proofs):
    """(f(t) - f(z)) h == sum_i (t_i - z_i) pi_i: the pairing equation of `check` (mod.rs:172-200) with the trapdoor in place of the
    pairing"""
    left = mul((mle_eval(evals, t) - mle_eval(evals, point)) % R, h)
    acc = _J_INF
    for ti, zi, pi in zip(t, point, proofs):
        acc = _j_add(acc, _j_from(mul((ti - zi) % R, pi)))
    return left == _j_affine(acc)


def pair_sums(level):
    return [add(level[2 * b], level[2 * b + 1]) for b in range(len(level) // 2)]
