"""CPU-only checks of the bodies behind MultilinearPC's setup (multilinear_pc/mod.rs:28-86): the eq table, the fixed-base window-table
multiplication and the batch normalisation over G1 and G2 of BLS12-381, the per-lane ladder and the pair sums that make the upper
levels -- compiled for the host by tests/emu/emu_ml_setup.cpp and stepped lane by lane, against tests/harness/g2ref.py.  Every
comparison is bit-exact on the Montgomery bytes.  The argument checks of the new entry points need no device either."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from harness import g2ref as G

HERE = os.path.dirname(os.path.abspath(__file__))
R = G.R
_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_ml_setup.so")
        srcs = [os.path.join(HERE, "emu", "emu_ml_setup.cpp")] + [
            os.path.join(HERE, "..", "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "ec.hpp", "fp32.hpp", "fp2.hpp", "g2.hpp", "ipa.hpp", "host_tail.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def eq_table(t):
    """L_0[x] = prod_j e(t_j, bit_j(x)), the product formula"""
    out = []
    for x in range(1 << len(t)):
        v = 1
        for j, tj in enumerate(t):
            v = v * (tj if (x >> j) & 1 else 1 - tj) % R
        out.append(v)
    return out


def trapdoors(nv, seed):
    """t vectors for nv variables: random ones, and ones drawn from {0, 1, r - 1, (r + 1) / 2} (mixed with random values)"""
    rnd = np.random.RandomState(seed)
    big = lambda: int.from_bytes(rnd.bytes(32), "little") % R
    special = [0, 1, R - 1, (R + 1) // 2]
    out = [[big() for _ in range(nv)], [special[(j + nv) % 4] for j in range(nv)], [special[j % 4] if j % 2 == 0 else big() for j in range(nv)]]
    out += [[s] * nv for s in special]
    return out


@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 6])
def test_eq_body_against_product_formula(nv):
    for t in trapdoors(nv, nv):
        out = np.zeros((1 << nv, 8), dtype=np.uint32)
        emu().emu_ml_eq(p32(G.scalars_array(t, True).view(np.uint32)), nv, p32(out))
        raw = out.view(np.uint8).reshape(-1, 32)
        assert all(int.from_bytes(bytes(row), "little") < R for row in raw), "a stored value is not canonical"
        got = G.scalars_from_array(raw, True)
        assert got == eq_table(t), t
        # the identity the upper levels rest on: pair sums of level 0 are the table of t[1:], and the whole table sums to 1
        if nv > 1:
            assert [(got[2 * b] + got[2 * b + 1]) % R for b in range(1 << (nv - 1))] == eq_table(t[1:])
        assert sum(got) % R == 1


def boundary_scalars():
    """both sides of the signed-digit boundary in the low window, a carry through 31 windows, every digit at the boundary, the top window"""
    rnd = np.random.RandomState(11)
    ks = [0, 1, 127, 128, 129, 255, 256, (1 << 248) - 1,
          int.from_bytes(b"\x80" * 31 + b"\x00", "little"), int.from_bytes(b"\x7f" * 31 + b"\x73", "little"),
          1 << 254, (R - 1) // 2, R - 128, R - 1]
    return ks + [int.from_bytes(rnd.bytes(32), "little") % R for _ in range(4)]


def fixed_base(group, base, ks, K):
    g1 = group == 1
    out = np.zeros((len(ks), 24 if g1 else 48), dtype=np.uint32)
    b = np.frombuffer(G.point_bytes(base, g1), dtype=np.uint32).copy()
    emu().emu_ml_fixed_base(group, p32(b), p32(G.scalars_array(ks, True).view(np.uint32)), C.c_size_t(len(ks)), K, p32(out))
    return [G.point_from_bytes(row.tobytes(), g1) for row in out]


@pytest.fixture(scope="module")
def h():
    return G.generator()


@pytest.fixture(scope="module")
def want_g2(h):
    ks = boundary_scalars()
    return ks, G.fixed_base(h).mul_many(ks)


def test_g2_table_mul_boundary_scalars(h, want_g2):
    ks, want = want_g2
    assert want[0] is G.INF and want[1] == h
    for K in (1, 8):
        assert fixed_base(2, h, ks, K) == want, K


def test_g2_ladder_boundary_scalars(h, want_g2):
    ks, want = want_g2
    assert fixed_base(2, h, ks, 0) == want


@pytest.mark.parametrize("K", [4, 8])
def test_g2_normalisation_run_lengths(h, want_g2, K):
    """n = K - 1, K, K + 1 and 2K + 1 with a zero scalar (an infinity, skipped in the prefix product) inside a run, at its start and at
    its end"""
    ks, want = want_g2
    pool = dict(zip(ks, want))
    nz = [k for k in ks if k]
    for n in (K - 1, K, K + 1, 2 * K + 1):
        for zero_at in (0, n // 2, n - 1):
            sel = [nz[(3 * i + n) % len(nz)] for i in range(n)]
            sel[zero_at] = 0
            assert fixed_base(2, h, sel, K) == [pool[k] for k in sel], (n, zero_at)
    assert fixed_base(2, h, [0] * (K + 1), K) == [G.INF] * (K + 1)


def test_g2_infinity_base(h):
    assert fixed_base(2, G.INF, [0, 1, R - 1, 12345], 4) == [G.INF] * 4
    assert fixed_base(2, G.INF, [0, 1, R - 1, 12345], 0) == [G.INF] * 4


def test_g1_instantiations_unchanged():
    """The generalised bodies over the G1 curve: the values of g2ref's own fixed-base multiplication, and word for word what the
    G1 emulation of the KZG setup path (emu_fixed_base_table, tests/emu/emu_msm.cpp) gives."""
    import test_emu_cpu as E
    g = G.g1_generator()
    ks = boundary_scalars()
    want = G.fixed_base(g).mul_many(ks)
    sc = G.scalars_array(ks, True).view(np.uint32)
    gb = np.frombuffer(G.point_bytes(g, True), dtype=np.uint32).copy()
    for K in (1, 5, 16):
        assert fixed_base(1, g, ks, K) == want, K
        old = np.zeros((len(ks), 24), dtype=np.uint32)
        E.emu().emu_fixed_base_table(0, p32(gb), p32(sc), C.c_size_t(len(ks)), K, p32(old))
        new = np.zeros((len(ks), 24), dtype=np.uint32)
        emu().emu_ml_fixed_base(1, p32(gb), p32(sc), C.c_size_t(len(ks)), K, p32(new))
        assert (old == new).all(), K
    assert fixed_base(1, g, ks, 0) == want


@pytest.mark.parametrize("nv", [1, 3, 4])
def test_levels_by_pair_sums_equal_the_reference_setup(nv, h):
    """The route of pc_hip_ml_setup on the host: level 0 by the table, every higher level by pair sums, for both groups -- against
    ml_setup_with_trapdoor, which multiplies every level.  t_0 = 0 and t_1 = 1 put infinities into the levels; t_2 = (r + 1) / 2
    makes every pair of level 2 a doubling."""
    rnd = np.random.RandomState(nv)
    t = [int.from_bytes(rnd.bytes(32), "little") % R for _ in range(nv)]
    cases = [t]
    if nv >= 3:
        cases.append([0, 1] + t[2:])
        cases.append(t[:2] + [(R + 1) // 2] + t[3:])
    for t in cases:
        pp = G.ml_setup_with_trapdoor(nv, t)
        for group, base, levels in ((1, pp["g"], pp["powers_of_g"]), (2, pp["h"], pp["powers_of_h"])):
            g1 = group == 1
            lvl = fixed_base(group, base, eq_table(t), 8)
            assert lvl == levels[0], (group, t)
            for i in range(1, nv + 1):
                arr = G.points_array(lvl, g1).view(np.uint32)
                out = np.zeros((len(lvl) // 2, arr.shape[1]), dtype=np.uint32)
                emu().emu_ml_pair_sums(group, p32(arr), C.c_size_t(len(lvl) // 2), 8, p32(out))
                lvl = [G.point_from_bytes(row.tobytes(), g1) for row in out]
                assert lvl == (levels[i] if i < nv else [base]), (group, i, t)


# ---- the built library, no device ---------------------------------------------------------------------------------------------

def test_argument_checks_need_no_device():
    from poly_commit_amd import _ffi
    lib = _ffi.load_library()
    INVALID, TOO_LARGE, UNSUPPORTED = -1, -5, -6
    buf = np.zeros(64, dtype=np.uint64)
    p_ = buf.ctypes.data_as(C.c_void_p)
    null = C.c_void_p(None)
    a, b = C.c_void_p(None), C.c_void_p(None)
    sz = C.c_size_t
    # NULL context, NULL pointers
    assert lib.pc_hip_ml_eq_evals(null, 0, p_, 3, p_) == INVALID
    assert lib.pc_hip_g2_fixed_base_batch_mul(null, 0, p_, p_, sz(1), p_) == INVALID
    assert lib.pc_hip_ml_setup(null, 0, 3, p_, p_, p_, C.byref(a), C.byref(b), None) == INVALID
    assert lib.pc_hip_ml_trim(null, null, null, 3, 2, C.byref(a), C.byref(b)) == INVALID
    assert lib.pc_hip_g2_srs_device_ptr(null) is None
    # A context that is never touched: every check below is made on the arguments alone, before the context is looked at.
    fake = np.zeros(1 << 16, dtype=np.uint8)
    ctx = fake.ctypes.data_as(C.c_void_p)
    assert lib.pc_hip_ml_eq_evals(ctx, 0, None, 3, p_) == INVALID
    assert lib.pc_hip_ml_eq_evals(ctx, 0, p_, 3, None) == INVALID
    assert lib.pc_hip_ml_eq_evals(ctx, 0, p_, 0, p_) == INVALID
    assert lib.pc_hip_ml_eq_evals(ctx, 0, p_, 31, p_) == TOO_LARGE
    assert lib.pc_hip_ml_eq_evals(ctx, 7, p_, 3, p_) == INVALID
    assert lib.pc_hip_ml_eq_evals(ctx, 1, p_, 3, p_) == UNSUPPORTED
    assert lib.pc_hip_g2_fixed_base_batch_mul(ctx, 0, None, p_, sz(1), p_) == INVALID
    assert lib.pc_hip_g2_fixed_base_batch_mul(ctx, 0, p_, None, sz(1), p_) == INVALID
    assert lib.pc_hip_g2_fixed_base_batch_mul(ctx, 0, p_, p_, sz(1), None) == INVALID
    assert lib.pc_hip_g2_fixed_base_batch_mul(ctx, 0, p_, p_, sz(1 << 31), p_) == TOO_LARGE
    assert lib.pc_hip_g2_fixed_base_batch_mul(ctx, 2, p_, p_, sz(1), p_) == UNSUPPORTED
    assert lib.pc_hip_ml_setup(ctx, 0, 0, p_, p_, p_, C.byref(a), C.byref(b), None) == INVALID
    assert lib.pc_hip_ml_setup(ctx, 0, 30, p_, p_, p_, C.byref(a), C.byref(b), None) == TOO_LARGE
    assert lib.pc_hip_ml_setup(ctx, 0, 3, None, p_, p_, C.byref(a), C.byref(b), None) == INVALID
    assert lib.pc_hip_ml_setup(ctx, 0, 3, p_, None, p_, C.byref(a), C.byref(b), None) == INVALID
    assert lib.pc_hip_ml_setup(ctx, 0, 3, p_, p_, None, C.byref(a), C.byref(b), None) == INVALID
    assert lib.pc_hip_ml_setup(ctx, 0, 3, p_, p_, p_, None, C.byref(b), None) == INVALID
    assert lib.pc_hip_ml_setup(ctx, 0, 3, p_, p_, p_, C.byref(a), None, None) == INVALID
    assert lib.pc_hip_ml_setup(ctx, 1, 3, p_, p_, p_, C.byref(a), C.byref(b), None) == UNSUPPORTED
    assert lib.pc_hip_ml_trim(ctx, None, None, 3, 2, C.byref(a), C.byref(b)) == INVALID
    assert a.value is None and b.value is None


def test_host_mirror_driver_compiles_and_links():
    """host/multilinear_pc.hpp with setup and the resident trim compiles and links against the library; the driver
    built here is the one the -m gpu test runs."""
    root = os.path.dirname(HERE)
    libdir = os.path.join(root, "poly_commit_amd")
    from poly_commit_amd import _ffi
    _ffi.load_library()
    exe = os.path.join(HERE, "cpp", "ml_setup_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
