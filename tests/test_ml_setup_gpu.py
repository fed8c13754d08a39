"""MultilinearPC's parameters made on the device (pc_hip_ml_eq_evals, pc_hip_g2_fixed_base_batch_mul, pc_hip_ml_setup, pc_hip_ml_trim)
against the restated reference tests/harness/g2ref.py (multilinear_pc/mod.rs:28-111).  Every comparison is bit-exact on canonical
Montgomery bytes.  Python builds whole keys only up to nv = 7; the case at nv = 16 is checked by closed forms."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from harness import g2ref as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = "bls12_381"
R = G.R
LADDER_BELOW = 4096          # abi_g2.hip FIXED_BASE_LADDER_BELOW: fewer scalars run the per-lane ladder
SLAB = 1 << 18               # abi_g2.hip FIXED_BASE_SLAB: results made and normalised per pass


def rand_fr(rnd, n):
    return [int.from_bytes(rnd.bytes(32), "little") % R for _ in range(n)]


def eq_table(t):
    """L[x] = prod_j e(t_j, bit_j(x)), the product formula"""
    out = []
    for x in range(1 << len(t)):
        v = 1
        for j, tj in enumerate(t):
            v = v * (tj if (x >> j) & 1 else 1 - tj) % R
        out.append(v)
    return out


def eq_at(t, x):
    v = 1
    for j, tj in enumerate(t):
        v = v * (tj if (x >> j) & 1 else 1 - tj) % R
    return v


def trapdoors(nv, seed):
    rnd = np.random.RandomState(seed)
    special = [0, 1, R - 1, (R + 1) // 2]
    out = [rand_fr(rnd, nv), [special[(j + nv) % 4] for j in range(nv)], [special[j % 4] if j % 2 == 0 else rand_fr(rnd, 1)[0] for j in range(nv)]]
    return out + [[s] * nv for s in special]


def boundary_scalars():
    """both sides of the signed-digit boundary in the low window, a carry through 31 windows, every digit at the boundary, the top
    window; 37 values in all"""
    rnd = np.random.RandomState(11)
    ks = [0, 1, 127, 128, 129, 255, 256, (1 << 248) - 1,
          int.from_bytes(b"\x80" * 31 + b"\x00", "little"), int.from_bytes(b"\x7f" * 31 + b"\x73", "little"),
          1 << 254, (R - 1) // 2, R - 128, R - 1]
    return ks + rand_fr(rnd, 37 - len(ks))


@functools.lru_cache(maxsize=None)
def pool37():
    ks = boundary_scalars()
    return ks, G.points_array(G.fixed_base(G.generator()).mul_many(ks))


@functools.lru_cache(maxsize=None)
def reference_params(nv, kind="random"):
    rnd = np.random.RandomState(500 + nv)
    t = rand_fr(rnd, nv)
    if kind == "zero-one":
        t[0], t[1] = 0, 1
    if kind == "half":
        t[2] = (R + 1) // 2
    return G.ml_setup_with_trapdoor(nv, t)


def g_bytes(pp):
    return np.frombuffer(G.point_bytes(pp["g"], True), dtype=np.uint8).copy()


def h_bytes(pp):
    return np.frombuffer(G.point_bytes(pp["h"]), dtype=np.uint8).copy()


def device_setup(ctx, pp):
    return ctx.ml_setup(CURVE, pp["nv"], g_bytes(pp), h_bytes(pp), G.scalars_array(pp["t"], True))


def g1_points(arr):
    return [G.point_from_bytes(row.tobytes(), True) for row in arr]


def g2_points(arr):
    return [G.point_from_bytes(row.tobytes()) for row in arr]


@pytest.mark.parametrize("nv", range(1, 8))
def test_eq_evals_against_product_formula(ctx, nv):
    import torch
    for t in trapdoors(nv, nv):
        out = torch.zeros((1 << nv, 32), dtype=torch.uint8, device="cuda")
        ctx.ml_eq_evals(CURVE, G.scalars_array(t, True), nv, out.data_ptr())
        raw = out.cpu().numpy()
        assert all(int.from_bytes(bytes(row), "little") < R for row in raw), "a stored value is not canonical"
        assert G.scalars_from_array(raw, True) == eq_table(t), t


@pytest.mark.parametrize("n", [1, 37, LADDER_BELOW - 1, LADDER_BELOW, SLAB + 3])
def test_g2_fixed_base_batch_mul(ctx, n):
    """The boundary scalars (n = 37: the per-lane ladder), both sides of the ladder / table switch, and one slab + 3 (the second pass
    of the table path holds three points): scalars periodic over the pool of 37, expected points the Python pool tiled."""
    import torch
    ks, want = pool37()
    idx = np.arange(n) % len(ks)
    sc = torch.from_numpy(np.ascontiguousarray(G.scalars_array(ks, True)[idx])).cuda()
    out = torch.zeros((n, 192), dtype=torch.uint8, device="cuda")
    ctx.g2_fixed_base_batch_mul(CURVE, h_bytes({"h": G.generator()}), sc.data_ptr(), n, out.data_ptr())
    got = out.cpu().numpy()
    assert not got[idx == 0].any()                                               # 0 * h: the all-zero encoding
    assert (got == want[idx]).all()


def check_setup(ctx, pp):
    import poly_commit_amd as pc
    nv = pp["nv"]
    gk, hk, mask = device_setup(ctx, pp)
    try:
        assert len(hk) == (2 << nv) - 1 and gk.n == (2 << nv) - 2
        for i in range(nv):
            off, m = pc.ml_level_offset(nv, i), 1 << (nv - i)
            assert g1_points(gk.read(off, m).view(np.uint8)) == pp["powers_of_g"][i], i
            assert g2_points(hk.read(off, m)) == pp["powers_of_h"][i], i
        assert g2_points(hk.read((2 << nv) - 2, 1)) == [pp["h"]]
        assert g1_points(mask) == [G.mul(ti, pp["g"]) for ti in pp["t"]]
    finally:
        gk.free()
        hk.free()


@pytest.mark.parametrize("nv", range(1, 8))
def test_setup_every_level_equals_the_reference(ctx, nv):
    check_setup(ctx, reference_params(nv))


def test_setup_with_infinities_in_the_levels(ctx):
    """t_0 = 0 and t_1 = 1: half of level 0 and half of level 1 are zero scalars"""
    pp = reference_params(5, "zero-one")
    assert sum(p is G.INF for p in pp["powers_of_h"][0]) == 24 and sum(p is G.INF for p in pp["powers_of_h"][1]) == 8
    check_setup(ctx, pp)


def test_setup_where_every_pair_of_a_level_is_a_doubling(ctx):
    """t_2 = (r + 1) / 2: e(t_2, 0) = e(t_2, 1), so the two points of every pair of level 2 are equal"""
    pp = reference_params(5, "half")
    lvl = pp["powers_of_h"][2]
    assert all(lvl[2 * b] == lvl[2 * b + 1] for b in range(len(lvl) // 2))
    check_setup(ctx, pp)


@pytest.fixture(scope="module")
def resident7(ctx):
    pp = reference_params(7)
    gk, hk, _ = device_setup(ctx, pp)
    yield pp, gk, hk
    gk.free()
    hk.free()


@pytest.mark.parametrize("supported", range(1, 8))
def test_trim_commit_open(ctx, resident7, supported):
    import poly_commit_amd as pc
    pp, gk, hk = resident7
    nv, s = pp["nv"], supported
    first = nv - s                                                               # the level that becomes level 0 of the trimmed key
    n = 1 << s
    srs, key = ctx.ml_trim(gk, hk, nv, s)
    old = pc.multilinear_pair_key(ctx, CURVE, [G.points_array(l) for l in pp["powers_of_h"][first:]])      # the host-parameter path
    try:
        assert srs.n == n and len(key) == n - 1
        assert g1_points(srs.read(0, n).view(np.uint8)) == pp["powers_of_g"][first]
        for i in range(s):
            assert g2_points(key.read(n - (n >> i), n >> (i + 1))) == G.pair_sums(pp["powers_of_h"][first + i]), i
        assert key.read(0, n - 1).tobytes() == old.read(0, n - 1).tobytes()
        # commit and open through the unchanged entry points
        rnd = np.random.RandomState(70 + s)
        evals, point = rand_fr(rnd, n), rand_fr(rnd, s)
        ev, pt = G.scalars_array(evals, True), G.scalars_array(point, True)
        comm, _ = srs.msm(ev.view(np.uint64), montgomery=True)
        t_sub = pp["t"][first:]
        assert G.point_from_bytes(comm.tobytes(), g1=True) == G.mul(G.mle_eval(evals, t_sub), pp["g"])
        out, _ = key.ml_open(ev, s, pt)
        assert G.ml_trapdoor_check(pp["h"], t_sub, evals, point, g2_points(out))
    finally:
        old.free()
        srs.free()
        key.free()


def test_trim_argument_checks(ctx, resident7):
    import poly_commit_amd as pc
    pp, gk, hk = resident7
    for nv, s in ((7, 0), (7, 8), (6, 3), (8, 3), (0, 0)):                       # supported out of range; keys that are not those of nv
        with pytest.raises(pc.PcHipError):
            ctx.ml_trim(gk, hk, nv, s)
    with pytest.raises(pc.PcHipError):
        ctx.ml_setup(CURVE, 0, g_bytes(pp), h_bytes(pp), G.scalars_array(pp["t"], True))
    with pytest.raises(pc.PcHipError):
        ctx.ml_setup("bn254", 3, g_bytes(pp), h_bytes(pp), G.scalars_array(pp["t"], True))


def test_setup_nv16_by_closed_forms(ctx):
    """A key Python cannot build (2^17 - 2 points per group; level 0 goes through the window table): f(t) g and f(t) h as MSMs over
    level 0, sum_x L_i[x] = 1 for every level of both groups, and sampled points of every level against the product formula."""
    import poly_commit_amd as pc
    import torch
    nv = 16
    n = 1 << nv
    rnd = np.random.RandomState(1616)
    t = rand_fr(rnd, nv)
    g, h = G.g1_generator(), G.generator()
    gk, hk, mask = ctx.ml_setup(CURVE, nv, g_bytes({"g": g}), h_bytes({"h": h}), G.scalars_array(t, True))
    try:
        ev = np.frombuffer(rnd.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
        ev[:, 31] &= 0x3f                                                        # Montgomery residues below 2^254 < r
        f_t = G.mle_eval(G.scalars_from_array(ev, True), t)
        ev_d = torch.from_numpy(ev).cuda()
        comm, _ = gk.msm(ev_d, n=n, montgomery=True)
        assert G.point_from_bytes(comm.tobytes(), g1=True) == G.mul(f_t, g)
        comm2, _ = hk.msm(ev_d, n=n, montgomery=True)
        assert G.point_from_bytes(comm2.tobytes()) == G.mul(f_t, h)
        ones = torch.from_numpy(np.ascontiguousarray(np.tile(G.scalars_array([1], True), (n, 1)))).cuda()
        g_arr, h_arr = G.point_bytes(g, True), G.point_bytes(h)
        xs, ks = [], []
        for i in range(nv):
            off, m = pc.ml_level_offset(nv, i), n >> i
            s1, _ = gk.msm(ones, n=m, base_offset=off, montgomery=True)
            s2, _ = hk.msm(ones, n=m, base_offset=off, montgomery=True)
            assert s1.tobytes() == g_arr and s2.tobytes() == h_arr, i
            for x in sorted(set([0, m - 1] + [int(v) for v in rnd.randint(0, m, 6)])):
                xs.append((i, off + x))
                ks.append(eq_at(t[i:], x))
        want_h = G.fixed_base(h).mul_many(ks)
        want_g = G.fixed_base(g).mul_many(ks)
        for (i, at), wh, wg in zip(xs, want_h, want_g):
            assert g2_points(hk.read(at, 1)) == [wh], (i, at)
            assert g1_points(gk.read(at, 1).view(np.uint8)) == [wg], (i, at)
        assert g2_points(hk.read(2 * n - 2, 1)) == [h]
        assert g1_points(mask[:2]) == [G.mul(t[0], g), G.mul(t[1], g)]
    finally:
        gk.free()
        hk.free()


def test_ledger_counts_the_keys_and_returns(ctx):
    pp = reference_params(6)
    nv = 6
    a, b, _ = device_setup(ctx, pp)                                              # (the call's grow-only scratch is made here)
    a.free()
    b.free()
    before = ctx.bytes_resident()
    gk, hk, _ = device_setup(ctx, pp)
    during = ctx.bytes_resident()
    g_b, h_b = ((2 << nv) - 2) * 96, ((2 << nv) - 1) * 192
    assert gk.bytes_resident()["bases"] == g_b and hk.bytes_resident()["bases"] == h_b
    assert during["keys"] - before["keys"] == g_b
    assert during["device_total"] - before["device_total"] == g_b + h_b
    assert during["n_keys"] - before["n_keys"] == 2
    srs, key = ctx.ml_trim(gk, hk, nv, 4)
    assert ctx.bytes_resident()["device_total"] - during["device_total"] == 16 * 96 + 15 * 192
    for k in (srs, key, gk, hk):
        k.free()
    assert ctx.bytes_resident() == before


def test_cpp_mirror_setup_trim_commit_open(tmp_path):
    """host/multilinear_pc.hpp: setup, trim from the resident parameters, commit and open in a process of its own (nv = 6, trimmed to 6
    and to 4 variables)."""
    libdir = os.path.join(ROOT, "poly_commit_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "ml_setup_driver")
    deps = [exe + ".cpp", os.path.join(libdir, "libpc_hip.so")] + [os.path.join(libdir, "host", f) for f in os.listdir(os.path.join(libdir, "host"))]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pp = reference_params(6)
    nv = 6
    for s in (6, 4):
        first = nv - s
        rnd = np.random.RandomState(60 + s)
        evals, point = rand_fr(rnd, 1 << s), rand_fr(rnd, s)
        sub = dict(nv=s, powers_of_g=pp["powers_of_g"][first:], powers_of_h=pp["powers_of_h"][first:])
        fin, fout = str(tmp_path / ("in%d.bin" % s)), str(tmp_path / ("out%d.bin" % s))
        with open(fin, "wb") as f:
            f.write(struct.pack("<II", nv, s))
            f.write(g_bytes(pp).tobytes() + h_bytes(pp).tobytes())
            f.write(G.scalars_array(pp["t"], True).tobytes())
            f.write(G.scalars_array(evals, True).tobytes())
            f.write(G.scalars_array(point, True).tobytes())
        res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        raw = open(fout, "rb").read()
        assert [G.point_from_bytes(raw[96 * i:96 * (i + 1)], g1=True) for i in range(nv)] == [G.mul(ti, pp["g"]) for ti in pp["t"]]
        raw = raw[96 * nv:]
        assert G.point_from_bytes(raw[:96], g1=True) == G.ml_commit(sub, evals)
        assert [G.point_from_bytes(raw[96 + 192 * i:96 + 192 * (i + 1)]) for i in range(s)] == G.ml_open(sub, evals, point)
