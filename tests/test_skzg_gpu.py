"""GPU suite of streaming_kzg (pc_hip_fold_tree, pc_hip_poly_div_multi, pc_hip_kzg_open_multi, pc_hip_kzg_batch_open_multi,
pc_hip_kzg_commit_folding, pc_hip_kzg_open_folding) against a true SRS of 4097 powers of a known tau: every result bit for bit
against the array definitions AND the streaming restatement of tests/harness/skzg.py (the group side through the trapdoor: a proof
over scalars s is (sum s[d] tau^d) G)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import pyref as R
from harness import skzg as S

pytestmark = pytest.mark.gpu
T = 1024                       # the fold / division tile in coefficients (csrc/skzg.hpp; test_tile_matches_the_library checks it)
N_SRS = 4097
SIZES = [1, 2, 3, 5, 8, T - 1, T, T + 1, 4097]


def _p(curve):
    return R.FIELDS[R.CURVES[curve]["fr"]]["p"]


def _scalars(curve, seed, n):
    return R.gen_scalars(R.CURVES[curve]["fr"], seed, n)


def _mont(curve, ints):
    return O.fr_mont_array(curve, list(ints)) if len(ints) else np.zeros((0, 4), dtype=np.uint64)


def _ints(curve, arr):
    return O.fr_from_mont_array(curve, np.ascontiguousarray(arr).reshape(-1, 4))


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


@functools.lru_cache(maxsize=None)
def _tau(curve):
    return _scalars(curve, 0x7A05, 1)[0]


@functools.lru_cache(maxsize=None)
def _g(curve):
    return R.gen_bases(curve, 1)[0]


def _point(curve, exponent):
    """exponent * G as the library's affine Montgomery words (all zero = infinity)"""
    return O.points_to_array(curve, [R.ec_mul(curve, exponent % _p(curve), _g(curve)) if exponent % _p(curve) else None])[0]


def _make_srs(ctx, curve):
    import torch
    tau_m = _mont(curve, [_tau(curve)])[0]
    pw = torch.empty((N_SRS, 4), dtype=torch.int64, device="cuda")
    ctx.fr_powers(curve, tau_m, N_SRS, pw.data_ptr())
    pts = torch.empty((N_SRS, 2 * O.fq_limbs(curve)), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(curve, O.points_to_array(curve, [_g(curve)])[0], pw.data_ptr(), N_SRS, pts.data_ptr())
    return ctx.upload_srs(curve, pts.data_ptr(), n=N_SRS)


@pytest.fixture(scope="module")
def srs381(ctx):
    srs = _make_srs(ctx, "bls12_381")
    yield srs
    srs.free()


@pytest.fixture(scope="module")
def srs254(ctx):
    srs = _make_srs(ctx, "bn254")
    yield srs
    srs.free()


def test_true_srs_points(srs381):
    for d in (0, 1, N_SRS - 1):
        assert (srs381.read(d, 1)[0] == _point("bls12_381", pow(_tau("bls12_381"), d, _p("bls12_381")))).all(), d


def _lg(n):
    return max(1, (n - 1).bit_length())


def _points3(curve):
    beta = _scalars(curve, 0xBE7A, 1)[0]
    p = _p(curve)
    return [beta * beta % p, beta, (-beta) % p]


def _points(curve, k):
    """k points: 0 among them (k >= 2), one repeated (k >= 3)"""
    pts = _scalars(curve, 0x9017 + k, k)
    if k >= 2:
        pts[1] = 0
    if k >= 3:
        pts[2] = pts[0]
    return pts


# ---- the folding tree -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("n", SIZES + [2 * T + 1])
def test_fold_tree_every_level(ctx, curve, n):
    import torch
    p = _p(curve)
    f = _scalars(curve, 0xF01D + n, n)
    fm = _mont(curve, f)
    for depth in sorted({1, _lg(n), _lg(n) + 2}):
        rhos = _scalars(curve, 0xF01E + depth, depth)
        want = S.fold_tree(f, rhos, p)
        total = sum(len(lv) for lv in want)
        for src in (fm, _dev(fm)):
            out = torch.full((total + 1, 4), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()      # torch's fill is only queued and the library's streams do not wait for torch's: finish it before the library writes
            offs = ctx.fold_tree(curve, src if isinstance(src, np.ndarray) else src.data_ptr(), _mont(curve, rhos), out.data_ptr(), total, n=n)
            assert offs == [sum(len(lv) for lv in want[:i]) for i in range(depth)]
            got = out.cpu().numpy().view(np.uint64)
            assert (got[total] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the last level"
            assert _ints(curve, got[:total]) == [c for lv in want for c in lv], (n, depth)
        with pytest.raises(Exception):
            ctx.fold_tree(curve, fm, _mont(curve, rhos), out.data_ptr(), total - 1, n=n)      # capacity below sum L_i


# ---- division by a vanishing polynomial -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
def test_poly_div_multi(ctx, curve, k):
    """lengths around k, the lanes' chunks (4), the groups (64), the tile, and past it the division scan's chunk (8) and fan-in
    (8 x 16 = 128, 8 x 256 = 2048) boundaries"""
    p = _p(curve)
    pts = _points(curve, k)
    zs = _mont(curve, pts)
    for n in sorted({1, k, k + 1, 2 * k, 3, 63, 64, 65, T - 1, T, T + 1, T + 127, T + 128, T + 129, 2047 + k, 2048 + k, 2049 + k, 4097}):
        f = _scalars(curve, 0xD17 + n, n)
        if n > 3:
            f[-1] = 0
        want_q, want_r = S.div_multi(f, pts, p)
        q, r = ctx.poly_div_multi(curve, _mont(curve, f), zs)
        assert _ints(curve, q) == want_q and _ints(curve, r) == want_r, (n, k)
        _, r2 = ctx.poly_div_multi(curve, _dev(_mont(curve, f)).data_ptr(), zs, n=n, want_quotient=False)      # device input, quotient_out NULL
        assert (r2 == r).all(), (n, k)


# ---- open_multi_points ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 5, 8, T - 1, T, T + 1, 4097])
def test_kzg_open_multi(ctx, srs381, n):
    curve = "bls12_381"
    p, tau = _p(curve), _tau(curve)
    f = _scalars(curve, 0x09E4 + n, n)
    pts = _points3(curve)
    proof, inf, rem = srs381.kzg_open_multi(_mont(curve, f), _mont(curve, pts))
    want_rem, want_e = S.open_multi(f, pts, tau, p)
    rem_a, e_a = S.space_open_multi_points(S.reversed_key(tau, N_SRS, p), list(reversed(f)), pts, p)
    assert (rem_a, e_a) == (want_rem, want_e)
    assert _ints(curve, rem) == want_rem and (proof == _point(curve, want_e)).all() and inf == (want_e == 0), n
    # one point: the single-point opening and the evaluation
    z = pts[1:2]
    proof1, inf1, rem1 = srs381.kzg_open_multi(_dev(_mont(curve, f)).data_ptr(), _mont(curve, z), n=n)
    single, sinf = srs381.kzg_open(_mont(curve, f), _mont(curve, z)[0])
    assert (proof1 == single).all() and inf1 == sinf
    assert (rem1[0] == ctx.poly_eval(curve, _mont(curve, f), _mont(curve, z)[0])).all()


def test_kzg_open_multi_edges(ctx, srs381):
    curve = "bls12_381"
    p, tau = _p(curve), _tau(curve)
    pts = _points3(curve)
    f = _scalars(curve, 0xED6E, 3)                                      # n = k: the zero quotient
    proof, inf, rem = srs381.kzg_open_multi(_mont(curve, f), _mont(curve, pts))
    assert inf and not proof.any() and _ints(curve, rem) == list(reversed(f))
    f = _scalars(curve, 0xED6F, 40)                                     # a base offset: the proof over powers 7 ..
    proof, _, _ = srs381.kzg_open_multi(_mont(curve, f), _mont(curve, pts), base_offset=7)
    assert (proof == _point(curve, S.msm_exponent(S.div_multi(f, pts, p)[0], tau, p, first=7))).all()
    import poly_commit_amd as pc
    with pytest.raises(pc.PcHipError):                                  # the key is shorter than the quotient
        srs381.kzg_open_multi(_mont(curve, _scalars(curve, 1, N_SRS + 4)), _mont(curve, pts))
    with pytest.raises(pc.PcHipError):
        srs381.kzg_open_multi(_mont(curve, f), _mont(curve, pts), base_offset=N_SRS - 30)


def test_kzg_batch_open_multi(ctx, srs381):
    """the reference's shape (streaming_kzg/tests.rs:86-126: 15 polynomials of degree 100, 5 points) with a 128-bit eta, and a ragged batch"""
    curve = "bls12_381"
    p, tau = _p(curve), _tau(curve)
    pts = _points(curve, 5)
    eta = _scalars(curve, 0xE7A, 1)[0] >> 127
    for lens in ([101] * 15, [101, 7, 1, 300, 5, 64]):
        polys = [_scalars(curve, 0xBA7C + j, ln) for j, ln in enumerate(lens)]
        want = _point(curve, S.batch_open_multi(polys, pts, eta, tau, p))
        proof, inf = srs381.kzg_batch_open_multi([_mont(curve, f) for f in polys], _mont(curve, pts), _mont(curve, [eta])[0])
        assert (proof == want).all() and not inf, lens
        devs = [_dev(_mont(curve, f)) for f in polys]
        proof_d, _ = srs381.kzg_batch_open_multi([d.data_ptr() for d in devs], _mont(curve, pts), _mont(curve, [eta])[0], lens=lens)
        assert (proof_d == want).all(), lens
    short = [_scalars(curve, 5, 4), _scalars(curve, 6, 5)]              # no polynomial longer than k: the identity
    proof, inf = srs381.kzg_batch_open_multi([_mont(curve, f) for f in short], _mont(curve, pts), _mont(curve, [eta])[0])
    assert inf and not proof.any()


# ---- commit_folding / open_folding --------------------------------------------------------------------------------------------------

def _check_commit_folding(srs, curve, f, depth):
    p, tau = _p(curve), _tau(curve)
    rhos = _scalars(curve, 0xC0F0 + depth, depth)
    want = S.commit_folding(f, rhos, tau, p)
    assert want == S.space_commit_folding(S.reversed_key(tau, N_SRS, p), list(reversed(f)), rhos, p)
    got, inf = srs.kzg_commit_folding(_mont(curve, f), _mont(curve, rhos))
    for i in range(depth):
        assert (got[i] == _point(curve, want[i])).all() and bool(inf[i]) == (want[i] == 0), (len(f), depth, i)
    return got, want


@pytest.mark.parametrize("n", SIZES)
def test_kzg_commit_folding(ctx, srs381, n):
    curve = "bls12_381"
    f = _scalars(curve, 0xC0FF + n, n)
    if n > 2:
        f[-1] = 0                                                       # a zero leading coefficient
    _check_commit_folding(srs381, curve, f, _lg(n))
    if n in (5, T + 1):
        _check_commit_folding(srs381, curve, f, _lg(n) + 2)


def test_kzg_commit_folding_zero_level_and_device_input(ctx, srs381):
    curve = "bls12_381"
    p = _p(curve)
    rho0 = _scalars(curve, 0xC0F0 + 3, 3)[0]
    # f[2b] = -rho_0 f[2b + 1]: level 1 (and every level below it) is all zero
    odd = _scalars(curve, 0x0DD, 4)
    f = [c for o in odd for c in ((-rho0 * o) % p, o)]
    got, want = _check_commit_folding(srs381, curve, f, 3)
    assert want == [0, 0, 0] and not got.any()
    g = _scalars(curve, 0x0DE, 2 * T + 3)
    rhos = _scalars(curve, 0xC0F0 + 5, 5)
    host, _ = srs381.kzg_commit_folding(_mont(curve, g), _mont(curve, rhos))
    dev, _ = srs381.kzg_commit_folding(_dev(_mont(curve, g)).data_ptr(), _mont(curve, rhos), n=len(g))
    assert (host == dev).all()


def _check_open_folding(srs, curve, n):
    p, tau = _p(curve), _tau(curve)
    depth = _lg(n)
    f = _scalars(curve, 0x0F01 + n, n)
    rhos, etas, pts = _scalars(curve, 0x0F02, depth), _scalars(curve, 0x0F03, depth), _points3(curve)
    want_rem, want_e = S.open_folding(f, rhos, pts, etas, tau, p)
    assert (want_rem, want_e) == S.space_open_folding(S.reversed_key(tau, N_SRS, p), list(reversed(f)), rhos, pts, etas, p)
    first, last = srs.read(0, 1), srs.read(N_SRS - 1, 1)
    args = (_mont(curve, f), _mont(curve, rhos), _mont(curve, pts), _mont(curve, etas))
    rem, proof, inf = srs.kzg_open_folding(*args)
    assert [_ints(curve, rem[i]) for i in range(depth)] == want_rem, n
    assert (proof == _point(curve, want_e)).all() and inf == (want_e == 0), n
    rem2, proof2, inf2 = srs.kzg_open_folding(*args)                    # again on the same key: identical
    assert (rem2 == rem).all() and (proof2 == proof).all() and inf2 == inf
    assert (srs.read(0, 1) == first).all() and (srs.read(N_SRS - 1, 1) == last).all()


@pytest.mark.parametrize("n", [5, T + 1, 4097])
def test_kzg_open_folding(ctx, srs381, n):
    _check_open_folding(srs381, "bls12_381", n)


def test_kzg_open_folding_short_levels_and_identity(ctx, srs381):
    """every level at most k long: all quotients empty, the proof is the identity and r_i = f_i zero-extended; device input"""
    curve = "bls12_381"
    p, tau = _p(curve), _tau(curve)
    f = _scalars(curve, 0x51, 6)
    rhos, etas, pts = _scalars(curve, 0x52, 4), _scalars(curve, 0x53, 4), _points3(curve)
    want_rem, want_e = S.open_folding(f, rhos, pts, etas, tau, p)
    rem, proof, inf = srs381.kzg_open_folding(_dev(_mont(curve, f)).data_ptr(), _mont(curve, rhos), _mont(curve, pts), _mont(curve, etas), n=6)
    assert want_e == 0 and inf and not proof.any()
    assert [_ints(curve, rem[i]) for i in range(4)] == want_rem


def test_bn254_commit_and_open_folding(ctx, srs254):
    curve = "bn254"
    f = _scalars(curve, 0x254, T + 1)
    _check_commit_folding(srs254, curve, f, _lg(T + 1))
    _check_open_folding(srs254, curve, T + 1)


def test_host_mirror_like_the_reference_tests():
    """host/streaming_kzg.hpp through tests/cpp/skzg_driver.cpp: time and space forms agree, one point = the single-point opening,
    remainders interpolate, commit_folding / open_folding against levels folded on the host"""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    libdir = os.path.join(os.path.dirname(here), "poly_commit_amd")
    exe = os.path.join(here, "cpp", "skzg_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "streaming_kzg host mirror OK" in r.stdout, r.stdout + r.stderr


# ---- residency, launches ------------------------------------------------------------------------------------------------------------

def test_calls_leave_nothing_resident(ctx, srs381):
    curve = "bls12_381"
    n = 4097
    f = _mont(curve, _scalars(curve, 0x4E5, n))
    depth = _lg(n)
    rhos, etas, pts = _mont(curve, _scalars(curve, 1, depth)), _mont(curve, _scalars(curve, 2, depth)), _mont(curve, _points3(curve))
    srs381.kzg_commit_folding(f, rhos)                                  # the key's pipelines exist from here on
    srs381.kzg_open_folding(f, rhos, pts, etas)
    ctx.trim()
    before = ctx.bytes_resident()
    srs381.kzg_commit_folding(f, rhos)
    srs381.kzg_open_folding(f, rhos, pts, etas)
    srs381.kzg_open_multi(f, pts)
    srs381.kzg_batch_open_multi([f, f[:100]], pts, etas[0])
    ctx.poly_div_multi(curve, f, pts)
    ctx.trim()
    assert ctx.bytes_resident() == before


def test_tile_matches_the_library_and_launch_counts(ctx, srs381):
    """one launch per level above the tile and one for all levels below; one launch for ALL short divisions"""
    curve = "bls12_381"
    n = 4097
    depth = _lg(n)
    f = _mont(curve, _scalars(curve, 0x1A, n))
    rhos, etas, pts = _mont(curve, _scalars(curve, 1, depth)), _mont(curve, _scalars(curve, 2, depth)), _mont(curve, _points3(curve))
    srs381.kzg_commit_folding(f, rhos)
    above = sum(1 for i in range(depth) if S.ceil_div(n, 1 << i) > T)
    assert ctx.last_skzg_launches() == (above + 1, 0)
    srs381.kzg_open_folding(f, rhos, pts, etas)
    tree, rest = ctx.last_skzg_launches()
    long_levels = [S.ceil_div(n, 1 << i) for i in range(1, depth + 1) if S.ceil_div(n, 1 << i) > T]
    assert tree == above + 1 and long_levels == [2049, 1025]

    def scan_sweeps(m):
        """levels of the division scan over m coefficients: chunks of 8, then fan-in 16, until one value is left"""
        levels, fan = 0, 8
        while True:
            m, levels, fan = S.ceil_div(m, fan), levels + 1, 16
            if m <= 1:
                return levels
    # the short levels' ONE launch; per long level three division scans (of L, L - 1, L - 2 coefficients), each level of a scan
    # swept up and down; the combination
    assert rest == 1 + sum(2 * scan_sweeps(ln - j) for ln in long_levels for j in range(3)) + 1
