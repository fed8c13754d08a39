"""CPU-only checks of the G2 code (fp2.hpp, the XYZZ law over Fq2, g2.hpp, MsmPlan<G2Of<C>>) compiled for the host by tests/emu/emu_g2.cpp
and stepped lane by lane, against the pure-Python reference tests/harness/g2ref.py.  Every comparison is bit-exact on the
Montgomery bytes.  The host utilities of the built library (pc_hip_g2_points_sum / pc_hip_g2_point_mul) and the argument checks
need no device either."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from harness import g2ref as G

HERE = os.path.dirname(os.path.abspath(__file__))
_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_g2.so")
        srcs = [os.path.join(HERE, "emu", "emu_g2.cpp")] + [
            os.path.join(HERE, "..", "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "ec.hpp", "fp32.hpp", "fp2.hpp", "g2.hpp", "host_tail.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        _emu.emu_g2_msm.restype = C.c_int
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def f2_bytes(a):
    return b"".join((v % G.P * G.MONT_Q % G.P).to_bytes(48, "little") for v in a)


def f2_arr(a):
    return np.frombuffer(f2_bytes(a), dtype=np.uint32).copy()


def f2_from(arr):
    b = arr.tobytes()
    ri = pow(G.MONT_Q, -1, G.P)
    return tuple(int.from_bytes(b[48 * i:48 * i + 48], "little") * ri % G.P for i in range(2))


def fop(op, a, b=(0, 0), c=(0, 0), d=(0, 0)):
    out = np.zeros(24, dtype=np.uint32)
    emu().emu_g2_fop(op, p32(f2_arr(a)), p32(f2_arr(b)), p32(f2_arr(c)), p32(f2_arr(d)), p32(out))
    raw = out.tobytes()
    assert all(int.from_bytes(raw[48 * i:48 * i + 48], "little") < G.P for i in range(2)), "a coefficient left [0, p)"
    return f2_from(out)


def test_fq2_arithmetic_against_python():
    """mul / sqr / add / sub / neg / inv / mul_add_mul over the edge values 0, 1, u, p - 1 in either coefficient and random elements.
    (No lazy forms are used in Fq2: every output coefficient is checked to be canonical.)"""
    P = G.P
    rnd = np.random.RandomState(7)
    big = lambda: int.from_bytes(rnd.bytes(48), "little") % P
    edge = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), (1, P - 1), (P - 1, 1), (1, 1)]
    vals = edge + [(big(), big()) for _ in range(6)]
    for a in vals:
        assert fop(1, a) == G.f2_sqr(a)
        assert fop(4, a) == G.f2_neg(a)
        assert fop(7, a) == G.f2_add(a, a)
        inv = fop(5, a)
        assert inv == G.f2_inv(a)
        if a != (0, 0):
            assert G.f2_mul(a, inv) == (1, 0)
        for b in vals:
            assert fop(0, a, b) == G.f2_mul(a, b)
            assert fop(2, a, b) == G.f2_add(a, b)
            assert fop(3, a, b) == G.f2_sub(a, b)
    for i, a in enumerate(vals):
        b, c, d = vals[(i + 3) % len(vals)], vals[(i + 7) % len(vals)], vals[(i + 11) % len(vals)]
        assert fop(6, a, b, c, d) == G.f2_mul_add_mul(a, b, c, d)


@pytest.fixture(scope="module")
def pts():
    g = G.generator()
    return G.fixed_base(g).mul_many([1, 2, 3, 0x1234567, G.R - 5, 77])


def ecop(op, zz, a, b, aux):
    out = np.zeros(48, dtype=np.uint32)
    arr = lambda p: np.frombuffer(G.point_bytes(p), dtype=np.uint32).copy()
    emu().emu_g2_ecop(op, zz, p32(arr(a)), p32(arr(b)), p32(arr(aux)), p32(out))
    return G.point_from_bytes(out.tobytes())


def test_g2_group_law_all_pairs(pts):
    """Every pair of {5 points, a negation, infinity} through the mixed and the full addition, with trivial and non-trivial ZZ:
    infinity on either side, P + P, P + (-P) included; the doublings too."""
    assert all(G.on_twist(p) for p in pts)
    five = pts[:5]
    cand = five + [G.neg(five[2]), G.INF]
    aux = pts[5]
    for zz in (0, 1):
        for a in cand:
            for b in cand:
                want = G.add(a, b)
                assert ecop(0, zz, a, b, aux) == want
                assert ecop(1, zz, a, b, aux) == want
            assert ecop(2, zz, a, a, aux) == G.add(a, a)
        # non-trivial ZZ through an aux point that collides with the operand
        assert ecop(1, 1, five[0], five[1], five[0]) == G.add(five[0], five[1])
    for a in cand:
        assert ecop(3, 0, a, a, aux) == G.add(a, a)


def run_msm(bases, scalars, n, base_off=0, c=0, T=0, T2=0, K0=0, mont=False):
    b = G.points_array(bases).view(np.uint32)
    s = G.scalars_array(scalars, mont).view(np.uint32)
    out = np.zeros(48, dtype=np.uint32)
    rc = emu().emu_g2_msm(p32(b), C.c_size_t(len(bases)), p32(s), C.c_size_t(n), base_off, c, T, T2, K0, int(mont), p32(out))
    assert rc == 0
    return G.point_from_bytes(out.tobytes())


@pytest.fixture(scope="module")
def key300():
    ks = [(i * 0x9e3779b97f4a7c15 + 12345) ** 3 % G.R for i in range(300)]
    return G.fixed_base(G.generator()).mul_many(ks)


SETTINGS = ((0, 0, 0, 0), (6, 4, 4, 2), (9, 7, 5, 4))


@pytest.mark.parametrize("n", [1, 2, 33, 300])
def test_g2_msm_stepped(key300, n):
    rnd = np.random.RandomState(n)
    ks = [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(n)]
    want = G.msm(key300[:n], ks)
    for (c, T, T2, K0) in SETTINGS:
        assert run_msm(key300[:n], ks, n, 0, c, T, T2, K0) == want, (c, T, T2, K0)
    assert run_msm(key300[:n], ks, n, 0, 0, 0, 0, 0, mont=True) == want
    if n > 2:      # a base offset, and fewer scalars than bases
        off = 3
        assert run_msm(key300[:n], ks[:n - off], n - off, off, 5, 4, 4, 2) == G.msm(key300[off:n], ks[:n - off])


def test_g2_msm_stepped_adversarial_scalars(key300):
    """The scalar sets of test_msm_stepped_adversarial_scalars (bucket collisions, huge buckets, signed-digit carries) on G2, with
    an infinity and a repeated base among the bases."""
    n = 300
    b = list(key300)
    b[5] = G.INF
    b[11] = b[10]
    rnd = np.random.RandomState(3)
    rk = [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(n)]
    cases = {
        "zeros": [0] * n,
        "ones": [1] * n,
        "r-1": [G.R - 1] * n,
        "same": [rk[0]] * n,
        "two-values": [rk[i % 2] for i in range(n)],
        "carry-chain": [((1 << 254) - 1 - i) % G.R for i in range(n)],
        "sparse": [rk[i] if i % 7 == 0 else 0 for i in range(n)],
    }
    for name, ks in cases.items():
        want = G.msm(b, ks)
        for (c, T, T2, K0) in SETTINGS:
            assert run_msm(b, ks, n, 0, c, T, T2, K0) == want, (name, c, T)


def test_g2_msm_stepped_partial_sums_cancel(key300):
    """The constructions of test_g2_msm_partial_sums_cancel_in_the_joins (tests/test_g2_msm_gpu.py) stepped on the host: 150 times P
    and 150 times -P under one scalar, in halves and alternating, sum to the identity (all-zero bytes) under every setting; with one
    -P turned into P the sum is 2k P.  (The stepped sort keeps index order inside a bucket: here `halves` makes non-trivial partial
    sums cancel in the joins and `alternating` with the even chunk length 4 makes every lane's own sum the identity.)  This pins the
    expected values and the plan's logic without a device: a failure of the device test then points at the HIP build."""
    n = 300
    P = key300[7]
    s = (0x9e3779b97f4a7c15 ** 4 + 21) % G.R
    pn = [P, G.neg(P)]
    layouts = {"halves": [i >= n // 2 for i in range(n)], "alternating": [bool(i & 1) for i in range(n)]}
    for name, minus in layouts.items():
        b = [pn[m] for m in minus]
        b2 = list(b)
        b2[[i for i in range(n) if minus[i]][n // 4]] = P
        for (c, T, T2, K0) in SETTINGS:
            assert run_msm(b, [s] * n, n, 0, c, T, T2, K0) is G.INF, (name, c, T)
            assert run_msm(b2, [s] * n, n, 0, c, T, T2, K0) == G.mul(2 * s, P), (name, c, T)


def test_g2_msm_stepped_one_base_one_scalar(key300):
    """test_g2_msm_equal_partial_sums_meet_in_the_joins stepped on the host: every partial sum of a bucket is the same point, the
    joins take the doubling branch of XyzzD::add over Fq2"""
    n = 300
    P = key300[2]
    for s in ((0x9e3779b97f4a7c15 ** 4 + 5) % G.R, 1, 3):
        want = G.mul(n * s % G.R, P)
        for (c, T, T2, K0) in SETTINGS:
            assert run_msm([P] * n, [s] * n, n, 0, c, T, T2, K0) == want, (s, c, T)


def test_g2_small_round_products(key300):
    """The per-lane scalar multiplication of the small-round kernel (g2.hpp ScalarMulBody), summed on the host."""
    for n in (1, 2, 17):
        ks = [0, 1, G.R - 1][:n] + [(i * 0xabcdef1234567 + 99) ** 4 % G.R for i in range(max(0, n - 3))]
        b = list(key300[:n])
        if n > 4:
            b[4] = G.INF
        out = np.zeros(48, dtype=np.uint32)
        emu().emu_g2_small_msm(p32(G.points_array(b).view(np.uint32)), p32(G.scalars_array(ks, True).view(np.uint32)), C.c_size_t(n), 1, p32(out))
        assert G.point_from_bytes(out.tobytes()) == G.msm(b, ks), n


def test_pair_sums_special_cases(key300):
    """P + P (a doubling), P + (-P) (an infinity in the output key), infinity inputs, for several lane lengths K."""
    p = key300
    pairs = [(p[0], p[1]), (p[2], p[2]), (p[3], G.neg(p[3])), (G.INF, p[4]), (p[5], G.INF), (G.INF, G.INF)] + [(p[10 + 2 * i], p[11 + 2 * i]) for i in range(13)]
    flat = [q for pr in pairs for q in pr]
    want = [G.add(a, b) for a, b in pairs]
    assert want[2] is G.INF and want[5] is G.INF
    for K in (1, 4, 8, 32):
        out = np.zeros((len(pairs), 48), dtype=np.uint32)
        emu().emu_g2_pair_sums(p32(G.points_array(flat).view(np.uint32)), C.c_size_t(len(pairs)), K, p32(out))
        got = [G.point_from_bytes(row.tobytes()) for row in out]
        assert got == want, K


@pytest.mark.parametrize("n_half", [1, 2, 63, 64, 65, 1000])
def test_ml_fold_against_python(n_half):
    rnd = np.random.RandomState(n_half)
    r = [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(2 * n_half)]
    r[0] = 0
    r[-1] = G.R - 1
    for z in (0, 1, G.R - 1, int.from_bytes(rnd.bytes(32), "little") % G.R):
        q, nxt = G.ml_fold(r, z)
        r_out = np.zeros((n_half, 8), dtype=np.uint32)
        q_out = np.zeros((n_half, 8), dtype=np.uint32)
        emu().emu_ml_fold(p32(G.scalars_array(r, True).view(np.uint32)), C.c_size_t(n_half), p32(G.scalars_array([z], True).view(np.uint32)),
                          p32(r_out), p32(q_out))
        assert G.scalars_from_array(r_out.view(np.uint8), True) == nxt
        assert G.scalars_from_array(q_out.view(np.uint8), True) == q


# ---- the built library, no device ---------------------------------------------------------------------------------------------

def test_library_host_utilities_and_argument_checks(key300):
    from poly_commit_amd import _ffi
    lib = _ffi.load_library()
    pts5 = key300[:5] + [G.INF, key300[2]]
    arr = G.points_array(pts5)
    out = np.zeros(192, dtype=np.uint8)
    assert lib.pc_hip_g2_points_sum(0, arr.ctypes.data_as(C.c_void_p), C.c_size_t(len(pts5)), out.ctypes.data_as(C.c_void_p)) == 0
    want = G.INF
    for p in pts5:
        want = G.add(want, p)
    assert G.point_from_bytes(out.tobytes()) == want
    for k in (0, 1, G.R - 1, 0x1234567890abcdef << 100):
        ks = G.scalars_array([k], True)
        assert lib.pc_hip_g2_point_mul(0, arr[1].ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        assert G.point_from_bytes(out.tobytes()) == G.mul(k, pts5[1])
    ks = G.scalars_array([5], True)
    p_, k_, o_ = arr.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    INVALID, UNSUPPORTED = -1, -6
    assert lib.pc_hip_g2_points_sum(0, None, C.c_size_t(2), o_) == INVALID
    assert lib.pc_hip_g2_points_sum(0, p_, C.c_size_t(2), None) == INVALID
    assert lib.pc_hip_g2_points_sum(7, p_, C.c_size_t(2), o_) == INVALID
    assert lib.pc_hip_g2_points_sum(-1, p_, C.c_size_t(2), o_) == INVALID
    assert lib.pc_hip_g2_point_mul(0, None, k_, o_) == INVALID
    assert lib.pc_hip_g2_point_mul(0, p_, None, o_) == INVALID
    assert lib.pc_hip_g2_point_mul(3, p_, k_, o_) == INVALID
    for curve in (1, 2):      # BN254, Pallas
        assert lib.pc_hip_g2_points_sum(curve, p_, C.c_size_t(2), o_) == UNSUPPORTED
        assert lib.pc_hip_g2_point_mul(curve, p_, k_, o_) == UNSUPPORTED
    # entry points that take a context refuse NULL before the device is touched
    null = C.c_void_p(None)
    handle = C.c_void_p(None)
    assert lib.pc_hip_g2_srs_upload(null, 0, p_, C.c_size_t(1), C.c_size_t(0), 0, C.byref(handle)) == INVALID
    assert lib.pc_hip_g2_msm(null, null, C.c_size_t(0), k_, 1, 0, C.c_size_t(1), o_, None) == INVALID
    assert lib.pc_hip_ml_fold(null, 0, null, C.c_size_t(1), k_, null, null) == INVALID
    assert lib.pc_hip_ml_open(null, null, k_, 0, 1, k_, o_, None) == INVALID
    assert lib.pc_hip_g2_srs_pair_sums(null, null, C.c_size_t(0), C.c_size_t(0), null, C.c_size_t(0)) == INVALID
    assert lib.pc_hip_g2_srs_len(null) == 0
    lib.pc_hip_g2_srs_free(null)
