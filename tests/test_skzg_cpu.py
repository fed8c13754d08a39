"""CPU suite of streaming_kzg: the two restatements of tests/harness/skzg.py agree -- (A) the reference's streaming algorithms
(streaming_kzg/space.rs, data_structures.rs) and (B) the array definitions of include/pc_hip.h --, the reference's pinned facts
(streaming_kzg/tests.rs:128-138, :194-258, the folding tests of data_structures.rs), the argument checks of the entry points with
no device, the kernels' tiles stepped on the host (tests/emu/emu_skzg.cpp), and the C++ mirror compiles."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref as R
from harness import skzg as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = R.FIELDS["bls12_381_fr"]["p"]
TAU = R.gen_scalars("bls12_381_fr", 0x7A0, 1)[0]


def _points(k, rnd):
    """k evaluation points with the cases that matter: 0 among them, one repeated (k >= 3)"""
    pts = [rnd.randrange(P) for _ in range(k)]
    if k >= 2:
        pts[1] = 0
    if k >= 3:
        pts[2] = pts[0]
    return pts


# ---- (A) == (B) ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_streaming_restatement_equals_array_definitions(k):
    rnd = random.Random(0x5C26 + k)
    pts = _points(k, rnd)
    for n in range(1, 41):
        f = [rnd.randrange(P) for _ in range(n)]
        if n % 7 == 3:
            f[-1] = 0                                             # a zero leading coefficient
        stream = list(reversed(f))
        key = S.reversed_key(TAU, 48, P)
        if n >= k:
            rem_a, proof_a = S.space_open_multi_points(key, stream, pts, P)
            rem_b, proof_b = S.open_multi(f, pts, TAU, P)
            assert rem_a == rem_b and proof_a == proof_b, (n, k)
            for z in pts:                                         # r interpolates p on the points
                assert S.evaluate_be(rem_b, z, P) == S.evaluate_le(f, z, P)
        for depth in range(1, 8):
            rhos = [rnd.randrange(P) for _ in range(depth)]
            etas = [rnd.randrange(P) for _ in range(depth)]
            levels = S.fold_tree(f, rhos, P)
            assert [len(lv) for lv in levels] == [S.ceil_div(n, 1 << i) for i in range(1, depth + 1)]
            # the tree iterator emits exactly the levels' coefficients, highest degree first within a level
            got = [[] for _ in range(depth)]
            for i, c in S.FoldedPolynomialTreeIter(stream, n, rhos, P):
                got[i - 1].append(c)
            assert [list(reversed(g)) for g in got] == levels, (n, depth)
            assert S.space_commit_folding(key, stream, rhos, P) == S.commit_folding(f, rhos, TAU, P), (n, depth)
            rem_a, proof_a = S.space_open_folding(key, stream, rhos, pts, etas, P)
            rem_b, proof_b = S.open_folding(f, rhos, pts, etas, TAU, P)
            assert rem_a == rem_b and proof_a == proof_b, (n, depth, k)


def test_division_is_k_synthetic_divisions_and_newton_remainder():
    """what the kernels compute: q = k successive divisions by (x - z_j); their remainders are the Newton coefficients of r"""
    rnd = random.Random(77)
    for n, k in ((7, 3), (5, 5), (3, 5), (40, 2), (1, 1)):
        f = [rnd.randrange(P) for _ in range(n)]
        pts = _points(k, rnd)
        cur, newton = list(f), []
        for z in pts:
            if not cur:
                newton.append(0)
                continue
            acc, out = 0, [0] * len(cur)
            for i in reversed(range(len(cur))):
                acc = (cur[i] + z * acc) % P
                out[i] = acc
            newton.append(out[0])
            cur = out[1:]
        r = [0] * k
        for j in reversed(range(k)):
            for d in reversed(range(1, k)):
                r[d] = (r[d - 1] - pts[j] * r[d]) % P
            r[0] = (newton[j] - pts[j] * r[0]) % P
        q, rem = S.div_multi(f, pts, P)
        assert cur == q and list(reversed(r)) == rem, (n, k)


# ---- the reference's pinned facts ---------------------------------------------------------------------------------------------

def test_open_multi_points_pinned_facts():
    """streaming_kzg/tests.rs:194-258"""
    stream = [80, 80, 88, 3, 73, 7, 24]                          # f = 80 x^6 + 80 x^5 + 88 x^4 + 3 x^3 + 73 x^2 + 7 x + 24
    beta = 53
    key = S.reversed_key(TAU, 201, P)
    remainder, _ = S.space_open_multi_points(key, stream, [beta * beta % P, beta, (-beta) % P], P)
    assert S.evaluate_be(remainder, beta, P) == 1807299544171
    assert S.evaluate_be(S.div_multi(list(reversed(stream)), [beta * beta % P, beta, (-beta) % P], P)[1], beta, P) == 1807299544171
    remainder, _ = S.space_open_multi_points(key, stream, [beta], P)
    assert len(remainder) == 1
    rnd = random.Random(1)
    poly = [rnd.randrange(P) for _ in range(101)]
    b = rnd.randrange(P)
    _, batch = S.space_open_multi_points(key, poly, [b], P)
    evaluation, single = S.space_open(key, poly, b, P)
    assert batch == single and evaluation == S.evaluate_be(poly, b, P)
    remainder, _ = S.space_open_multi_points(key, poly, [b, (-b) % P, b * b % P], P)
    assert S.evaluate_be(remainder, b, P) == S.evaluate_be(poly, b, P)
    assert S.evaluate_be(remainder, b * b % P, P) == S.evaluate_be(poly, b * b % P, P)
    # the array form of the same: one point gives the single-point opening
    f = list(reversed(poly))
    assert S.open_multi(f, [b], TAU, P) == ([evaluation], single)
    assert single == S.msm_exponent(R.witness_polynomial("bls12_381_fr", f, b), TAU, P)


def test_vanishing_polynomial():
    """streaming_kzg/tests.rs:128-138"""
    zeros = S.vanishing_polynomial([10, 5, 13], P)
    assert len(zeros) == 4 and zeros[-1] == 1
    assert [S.evaluate_le(zeros, x, P) for x in (10, 5, 13)] == [0, 0, 0]


def test_folded_polynomial_tree():
    """the two folding tests at the end of streaming_kzg/data_structures.rs"""
    it = S.FoldedPolynomialTreeIter([1, 2, 1, 1], 4, [1, 2], P)
    assert [next(it), next(it), next(it)] == [(1, 3), (1, 2), (2, 2 + 2 * 3)]
    items = list(S.FoldedPolynomialTreeIter([1] * 12, 12, [1] * 4, P))
    assert items[5] == (1, 2) and items[-1] == (4, 12)
    assert S.fold_tree([1] * 12, [1] * 4, P)[-1] == [12]
    # the stream of the last level alone has ceil(n / 2^depth) items
    assert len(S.fold_tree([1, 1, 2, 1], [1, 2], P)[-1]) == 1 and S.fold_tree([1, 1, 2, 1], [1, 2], P)[-1][0] == 2 + 2 * 3


# ---- the entry points' argument checks, with no device ------------------------------------------------------------------------

def test_argument_validation_needs_no_device():
    from poly_commit_amd import _ffi
    lib = _ffi.load_library()
    INVALID, TOO_LARGE = -1, -5
    buf = np.zeros(64, dtype=np.uint64)
    p_ = buf.ctypes.data_as(C.c_void_p)
    szs = (C.c_size_t * 4)(5, 5, 5, 5)
    ptrs = (C.c_void_p * 4)(*([buf.ctypes.data] * 4))
    inf = (C.c_int * 8)()
    sz = C.c_size_t
    # a context and a key that are never touched: every check below is made on the arguments alone.  (The zeroed key belongs to no
    # context, so a call that passes those checks ends at the key check: PC_ERR_INVALID_ARG as well, still without a device.)
    fake = np.zeros(1 << 16, dtype=np.uint8)
    ctx = fake.ctypes.data_as(C.c_void_p)
    fake_key = np.zeros(1 << 12, dtype=np.uint8)
    key = fake_key.ctypes.data_as(C.c_void_p)

    def fold_tree(c=ctx, curve=0, co=p_, n=5, ch=p_, depth=3, out=p_, cap=64, offs=szs):
        return lib.pc_hip_fold_tree(c, curve, co, 0, sz(n), ch, sz(depth), out, sz(cap), offs)
    assert [fold_tree(c=None), fold_tree(co=None), fold_tree(ch=None), fold_tree(out=None), fold_tree(offs=None)] == [INVALID] * 5
    assert [fold_tree(n=0), fold_tree(depth=0), fold_tree(curve=4), fold_tree(curve=-1)] == [INVALID] * 4
    assert fold_tree(cap=3 + 2 + 1 - 1) == INVALID                                  # sum L_i = 3 + 2 + 1
    assert fold_tree(n=1 << 32) == TOO_LARGE and fold_tree(depth=65) == TOO_LARGE

    def div(c=ctx, curve=0, co=p_, n=5, z=p_, k=3, q=p_, r=p_):
        return lib.pc_hip_poly_div_multi(c, curve, co, 0, sz(n), z, sz(k), q, 0, r)
    assert [div(c=None), div(co=None), div(z=None), div(r=None), div(n=0), div(k=0), div(curve=9)] == [INVALID] * 7
    assert div(k=17) == TOO_LARGE and div(n=1 << 32) == TOO_LARGE

    def open_multi(c=ctx, s=key, co=p_, n=5, z=p_, k=3, out=p_):
        return lib.pc_hip_kzg_open_multi(c, s, sz(0), co, 0, sz(n), z, sz(k), None, out, inf)
    assert [open_multi(c=None), open_multi(s=None), open_multi(co=None), open_multi(z=None), open_multi(out=None)] == [INVALID] * 5
    assert [open_multi(n=0), open_multi(k=0), open_multi(n=2, k=3), open_multi()] == [INVALID] * 4
    assert open_multi(k=17, n=20) == TOO_LARGE and open_multi(n=1 << 32) == TOO_LARGE

    def batch(c=ctx, s=key, polys=ptrs, lens=szs, count=4, z=p_, k=3, eta=p_, out=p_):
        return lib.pc_hip_kzg_batch_open_multi(c, s, sz(0), polys, 0, lens, sz(count), z, sz(k), eta, out, inf)
    assert [batch(c=None), batch(s=None), batch(polys=None), batch(lens=None), batch(z=None), batch(eta=None), batch(out=None)] == [INVALID] * 7
    assert [batch(count=0), batch(k=0), batch()] == [INVALID] * 3
    assert batch(k=17) == TOO_LARGE
    assert batch(polys=(C.c_void_p * 4)(buf.ctypes.data, None, buf.ctypes.data, buf.ctypes.data)) == INVALID

    def commit_folding(c=ctx, s=key, co=p_, n=5, ch=p_, depth=3, out=p_):
        return lib.pc_hip_kzg_commit_folding(c, s, sz(0), co, 0, sz(n), ch, sz(depth), out, inf)
    assert [commit_folding(c=None), commit_folding(s=None), commit_folding(co=None), commit_folding(ch=None), commit_folding(out=None)] == [INVALID] * 5
    assert [commit_folding(n=0), commit_folding(depth=0), commit_folding()] == [INVALID] * 3
    assert commit_folding(n=1 << 32) == TOO_LARGE and commit_folding(depth=65) == TOO_LARGE

    def open_folding(c=ctx, s=key, co=p_, n=5, ch=p_, depth=3, z=p_, k=3, etas=p_, rem=p_, out=p_):
        return lib.pc_hip_kzg_open_folding(c, s, sz(0), co, 0, sz(n), ch, sz(depth), z, sz(k), etas, rem, out, inf)
    assert [open_folding(c=None), open_folding(s=None), open_folding(co=None), open_folding(ch=None), open_folding(z=None), open_folding(etas=None),
            open_folding(rem=None), open_folding(out=None)] == [INVALID] * 8
    assert [open_folding(n=0), open_folding(depth=0), open_folding(k=0), open_folding()] == [INVALID] * 4
    assert open_folding(k=17) == TOO_LARGE and open_folding(n=1 << 32) == TOO_LARGE and open_folding(depth=65) == TOO_LARGE
    assert lib.pc_hip_last_skzg_launches(None, None) == INVALID


# ---- the kernels' tiles stepped on the host -------------------------------------------------------------------------------------

_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_skzg.so")
        srcs = [os.path.join(HERE, "emu", "emu_skzg.cpp")] + [os.path.join(ROOT, "poly_commit_amd", "csrc", f) for f in ("skzg.hpp", "poly.hpp", "fp32.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        _emu.emu_skzg_tile.restype = C.c_uint32
        _emu.emu_skzg_fold_tree.restype = C.c_uint32
        _emu.emu_skzg_div_multi.restype = C.c_uint32
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def test_tile_is_what_the_abi_sizes_its_scratch_for():
    src = open(os.path.join(ROOT, "poly_commit_amd", "csrc", "pc_internal.hpp")).read()
    assert "constexpr uint32_t SKZG_TILE = %d;" % emu().emu_skzg_tile() in src


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_fold_tree_stepped(curve):
    """every level, around the tile: one coefficient below it, at it, above it (one pair launch, then the tail), and three pair
    launches; depth below, at and past log2 n"""
    T = emu().emu_skzg_tile()
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    for n in (1, 2, 3, 5, 8, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3):
        f = R.gen_scalars(fr, 0xF01D + n, n)
        if n > 2:
            f[-1] = 0
        lg = max(1, (n - 1).bit_length())
        for depth in sorted({1, lg, lg + 2}):
            rhos = R.gen_scalars(fr, 0xF01E + depth, depth)
            want = S.fold_tree(f, rhos, p)
            offs = np.cumsum([0] + [len(lv) for lv in want], dtype=np.uint64)
            out = np.zeros((int(offs[-1]) + 1, 4), dtype=np.uint64)
            out[-1] = 0xA5
            launches = emu().emu_skzg_fold_tree(O.CURVES[curve], p32(O.fr_mont_array(curve, f).view(np.uint32)), C.c_size_t(n),
                                                p32(O.fr_mont_array(curve, rhos).view(np.uint32)), depth, p32(out.view(np.uint32)),
                                                offs.ctypes.data_as(C.POINTER(C.c_uint64)))
            got = O.fr_from_mont_array(curve, out[:-1])
            assert [got[int(offs[i]):int(offs[i + 1])] for i in range(depth)] == want, (n, depth)
            assert (out[-1] == 0xA5).all(), "written past the last level"
            above = sum(1 for i in range(depth) if S.ceil_div(n, 1 << i) > T)      # levels whose SOURCE is longer than a tile
            assert launches == above + (1 if depth > above else 0), (n, depth)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
def test_division_stepped(curve, k):
    """all polynomials of one call at once, as pc_hip_kzg_open_folding divides its levels: lengths around k, around the lanes'
    chunks (4), the groups (64) and the tile, and two longer than the tile (the division scan: chunk 8, fan-in 16)"""
    T = emu().emu_skzg_tile()
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    rnd = random.Random(k)
    pts = [rnd.randrange(p) for _ in range(k)]
    if k >= 2:
        pts[1] = 0
    if k >= 3:
        pts[2] = pts[0]
    lens = sorted({1, 2, k, k + 1, 2 * k, 3, 4, 5, 63, 64, 65, 255, 257, T - 1, T, T + 1, T + 130})
    polys = [R.gen_scalars(fr, 0xD17 + n, n) for n in lens]
    polys[-2][-1] = 0
    arrs = [O.fr_mont_array(curve, f) for f in polys]
    quots = [np.zeros((max(n - k, 0) + 1, 4), dtype=np.uint64) for n in lens]
    rems = np.zeros((len(lens), k, 4), dtype=np.uint64)
    launches = emu().emu_skzg_div_multi(O.CURVES[curve], (C.c_void_p * len(lens))(*[a.ctypes.data for a in arrs]), (C.c_uint32 * len(lens))(*lens),
                                        C.c_size_t(len(lens)), p32(O.fr_mont_array(curve, pts).view(np.uint32)), k,
                                        (C.c_void_p * len(lens))(*[q.ctypes.data for q in quots]), p32(rems.view(np.uint32)))
    for i, (n, f) in enumerate(zip(lens, polys)):
        q, r = S.div_multi(f, pts, p)
        assert O.fr_from_mont_array(curve, quots[i][:max(n - k, 0)]) == q, (n, k)
        assert O.fr_from_mont_array(curve, rems[i]) == r, (n, k)
    assert launches >= 1 + 2 * k * 2                                               # one launch for every short one, the scans of the two long ones


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

def test_host_mirror_driver_compiles_and_links():
    """host/streaming_kzg.hpp compiles and links against the library; the driver built here is the one the -m gpu test runs"""
    from poly_commit_amd import _ffi
    _ffi.load_library()
    libdir = os.path.join(ROOT, "poly_commit_amd")
    exe = os.path.join(HERE, "cpp", "skzg_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no HIP device" in r.stdout
