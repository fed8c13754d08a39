"""The restated MultilinearPC of tests/harness/g2ref.py (multilinear_pc/mod.rs:28-168) against itself by the trapdoor: the key is built
from a known t, and each opening must satisfy (f(t) - f(z)) h == sum_i (t_i - z_i) pi_i in G2 -- the pairing equation of `check`
(mod.rs:172-200) with the trapdoor in place of the pairing.  This pins the restated `open` independently of the device."""
import numpy as np
import pytest

from harness import g2ref as G


def rand_fr(rnd, n):
    return [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(n)]


def test_generator_is_a_point_of_order_r_on_the_twist():
    g = G.generator()
    assert g is not G.INF and G.on_twist(g)
    assert G.mul(G.R, g, mod_r=False) is G.INF
    assert G.mul(G.R - 1, g) == G.neg(g)


@pytest.mark.parametrize("nv", range(1, 9))
def test_open_satisfies_the_trapdoor_identity(nv):
    rnd = np.random.RandomState(100 + nv)
    t = rand_fr(rnd, nv)
    ck = G.ml_setup_with_trapdoor(nv, t)
    assert [len(l) for l in ck["powers_of_h"]] == [1 << (nv - i) for i in range(nv)]
    evals = rand_fr(rnd, 1 << nv)
    point = rand_fr(rnd, nv)
    proofs = G.ml_open(ck, evals, point)
    assert len(proofs) == nv and all(G.on_twist(p) for p in proofs)
    assert G.ml_trapdoor_check(ck["h"], t, evals, point, proofs)
    # the commitment is f(t) g: the key's level 0 holds eq(t, x) g
    assert G.ml_commit(ck, evals) == G.mul(G.mle_eval(evals, t), ck["g"])
    # a wrong proof does not pass
    bad = list(proofs)
    bad[0] = G.add(bad[0], ck["h"])
    assert not G.ml_trapdoor_check(ck["h"], t, evals, point, bad)
    # the pair-sum form the device uses gives the same proofs: every q[b] multiplies H[2b] + H[2b + 1]
    r = list(evals)
    for i in range(nv):
        q, r = G.ml_fold(r, point[i])
        assert G.msm(G.pair_sums(ck["powers_of_h"][i]), q) == proofs[i]


def test_host_mirror_compiles_and_links():
    """host/multilinear_pc.hpp (trim / commit / open above the C ABI) compiles and links against the library; the driver built here is
    the one the -m gpu test runs."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "poly_commit_amd")
    if not os.path.exists(os.path.join(libdir, "libpc_hip.so")):
        import importlib
        importlib.import_module("poly_commit_amd.build").build()
    exe = os.path.join(root, "tests", "cpp", "multilinear_pc_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
