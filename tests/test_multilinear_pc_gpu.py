"""MultilinearPC on the device (pc_hip_msm for commit, pc_hip_ml_open / pc_hip_ml_fold + pc_hip_g2_msm for open) against the restated
reference tests/harness/g2ref.py (multilinear_pc/mod.rs:28-168), bit-exact; the trapdoor identity is checked on the device's proofs."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from harness import g2ref as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = "bls12_381"


def rand_fr(rnd, n):
    return [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(n)]


def make_case(nv, seed=0):
    rnd = np.random.RandomState(1000 + nv + seed)
    t = rand_fr(rnd, nv)
    ck = G.ml_setup_with_trapdoor(nv, t)
    evals, point = rand_fr(rnd, 1 << nv), rand_fr(rnd, nv)
    return t, ck, evals, point


def proofs_of(out):
    return [G.point_from_bytes(row.tobytes()) for row in out]


def build_driver():
    libdir = os.path.join(ROOT, "poly_commit_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "multilinear_pc_driver")
    src = exe + ".cpp"
    deps = [src, os.path.join(libdir, "libpc_hip.so")] + [os.path.join(libdir, "host", f) for f in os.listdir(os.path.join(libdir, "host"))]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src, "-L" + libdir, "-lpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("nv", range(1, 11))
def test_commit_and_open_against_the_reference(ctx, nv, tmp_path):
    import torch
    import poly_commit_amd as pc
    t, ck, evals, point = make_case(nv)
    want_comm = G.ml_commit(ck, evals)
    want = G.ml_open(ck, evals, point)
    assert G.ml_trapdoor_check(ck["h"], t, evals, point, want)
    n = 1 << nv
    g_arr = G.points_array(ck["powers_of_g"][0], g1=True)
    h_arrs = [G.points_array(l) for l in ck["powers_of_h"]]
    ev, pt = G.scalars_array(evals, True), G.scalars_array(point, True)
    srs = ctx.upload_srs(CURVE, g_arr.view(np.uint64))
    key = pc.multilinear_pair_key(ctx, CURVE, h_arrs)
    try:
        assert len(key) == n - 1
        # the resident key is the pair sums of every level
        for i in range(nv):
            got = key.read(n - (n >> i), n >> (i + 1))
            assert proofs_of(got) == G.pair_sums(ck["powers_of_h"][i]), i
        comm, _ = srs.msm(ev.view(np.uint64), montgomery=True)
        assert G.point_from_bytes(comm.tobytes(), g1=True) == want_comm
        out, inf = key.ml_open(ev, nv, pt)                                        # host evaluations
        got = proofs_of(out)
        assert got == want and inf == [p is G.INF for p in want]
        assert G.ml_trapdoor_check(ck["h"], t, evals, point, got)                  # the identity on the device's proofs
        out_d, _ = key.ml_open(torch.from_numpy(ev).cuda(), nv, pt)               # device evaluations
        assert proofs_of(out_d) == want
        # the rounds driven one by one: pc_hip_ml_fold + pc_hip_g2_msm
        r = torch.from_numpy(ev).cuda()
        for i in range(nv):
            half = n >> (i + 1)
            r_out = torch.empty((half, 32), dtype=torch.uint8, device="cuda")
            q = torch.empty((half, 32), dtype=torch.uint8, device="cuda")
            ctx.ml_fold(CURVE, r.data_ptr(), half, pt[i], r_out.data_ptr(), q.data_ptr())
            pi, _ = key.msm(q, n=half, base_offset=n - (n >> i), montgomery=True)
            assert G.point_from_bytes(pi.tobytes()) == want[i], i
            r = r_out
        assert G.scalars_from_array(r.cpu().numpy(), True) == [G.mle_eval(evals, point)]
    finally:
        key.free()
        srs.free()
    # the C++ host mirror (host/multilinear_pc.hpp): trim, commit, open in a process of its own
    exe = build_driver()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", nv))
        f.write(g_arr.tobytes())
        for a in h_arrs:
            f.write(a.tobytes())
        f.write(ev.tobytes())
        f.write(pt.tobytes())
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = open(fout, "rb").read()
    assert G.point_from_bytes(raw[:96], g1=True) == want_comm
    assert [G.point_from_bytes(raw[96 + 192 * i:96 + 192 * (i + 1)]) for i in range(nv)] == want


CHILD = r'''
import sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import poly_commit_amd as pc
d = np.load(sys.argv[1])
ctx = pc.Context(0)
nv = int(d["nv"])
key = pc.multilinear_pair_key(ctx, "bls12_381", [d["h%d" % i] for i in range(nv)])
out, inf = key.ml_open(np.ascontiguousarray(d["ev"]), nv, np.ascontiguousarray(d["pt"]))
key.free()
ctx.close()
print("PROOFS " + out.tobytes().hex())
'''


@pytest.mark.parametrize("small", ["0", "3", "32", "128"])
def test_open_on_both_sides_of_the_small_round_threshold(small, tmp_path):
    """PC_HIP_G2_SMALL_ROUND (read once per process: hence the subprocess): 0 = every round through the full pipeline, 128 = the last
    eight rounds as one small kernel each; the proofs do not depend on it."""
    nv = 9
    _, ck, evals, point = make_case(nv, seed=7)
    want = G.ml_open(ck, evals, point)
    f = str(tmp_path / "case.npz")
    np.savez(f, nv=nv, ev=G.scalars_array(evals, True), pt=G.scalars_array(point, True), **{"h%d" % i: G.points_array(l) for i, l in enumerate(ck["powers_of_h"])})
    env = dict(os.environ, PC_HIP_G2_SMALL_ROUND=small)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD, f], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "PROOFS " in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw = bytes.fromhex(r.stdout.split("PROOFS ")[1].split()[0])
    assert [G.point_from_bytes(raw[192 * i:192 * (i + 1)]) for i in range(nv)] == want


def test_all_zero_polynomial_gives_infinities(ctx):
    import poly_commit_amd as pc
    nv = 6
    _, ck, _, point = make_case(nv)
    key = pc.multilinear_pair_key(ctx, CURVE, [G.points_array(l) for l in ck["powers_of_h"]])
    try:
        out, inf = key.ml_open(np.zeros((1 << nv, 32), dtype=np.uint8), nv, G.scalars_array(point, True))
        assert not out.any() and inf == [True] * nv
    finally:
        key.free()


def test_open_nv20_on_periodic_keys(ctx):
    """powers_of_h[i][x] = pool[(x + i) mod 1024], a pool of 1024 Python-made points with two equal neighbours: the pair sums contain
    doublings, every pair sum repeats 2^(9 - i) times in its level (huge buckets), and the level offset shifts which points pair up.
    Expected proofs: Python MSMs over the pool with the reference's scalars summed per residue."""
    import poly_commit_amd as pc
    nv, m = 20, 1024
    n = 1 << nv
    ks = [(i * 0x9e3779b97f4a7c15 + 0x1234567) ** 3 % G.R for i in range(m)]
    pool = G.fixed_base(G.generator()).mul_many(ks)
    pool[5] = pool[4]                                                            # equal neighbours: a doubling among the pair sums
    pool_arr = G.points_array(pool)
    levels = []
    for i in range(nv):
        size = n >> i
        idx = (np.arange(size) + i) % m
        levels.append(np.ascontiguousarray(pool_arr[idx]))
    key = pc.multilinear_pair_key(ctx, CURVE, levels)
    del levels
    rnd = np.random.RandomState(2020)
    ev = np.frombuffer(rnd.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    ev[:, 31] &= 0x3f                                                            # Montgomery residues below 2^254 < r
    point = rand_fr(rnd, nv)
    rinv = pow(G.MONT_R, -1, G.R)
    r = [int.from_bytes(row.tobytes(), "little") * rinv % G.R for row in ev]
    try:
        out, inf = key.ml_open(ev, nv, G.scalars_array(point, True))
        got = proofs_of(out)
        for i in range(nv):
            q, r = G.ml_fold(r, point[i])
            per = [0] * m
            for x in range(n >> i):                                              # the reference's scalars[x] = q[x >> 1] over ALL points of the level
                per[(x + i) % m] += q[x >> 1]
            want = G.msm(pool, [v % G.R for v in per])
            assert got[i] == want and inf[i] == (want is G.INF), i
    finally:
        key.free()
