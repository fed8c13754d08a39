"""Key validation without a GPU: the reference (tests/harness/swvalidate.py) against the facts of the curves, the generated constants of
the fast subgroup test (csrc/validate_constants.h) against tools/gen_constants.py and those facts, and the bodies of csrc/validate.hpp
as compiled by g++ (the host build of tests/hip/probe_validate.hip) against the reference on the whole adversarial set: this is where
a wrong cube root, or a clause of the shortcut that is unsound on some torsion component, shows."""
import importlib.util
import os

import numpy as np
import pytest

from harness import swvalidate as V

S, R = V.S, V.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen_constants():
    spec = importlib.util.spec_from_file_location("_gen_constants_validate", os.path.join(ROOT, "tools", "gen_constants.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_curve_parameters():
    """the published x of the two curves, recovered from the moduli, and h = (x - 1)^2 / 3"""
    assert V.bls12_x("bls12_381") == -0xd201000000010000 and V.bls12_x("bls12_377") == 0x8508c00000000001
    for curve in V.BLS12:
        x, (p, r, _) = V.bls12_x(curve), R.curve_params(curve)
        assert S.cofactor(curve) * r == p + 1 - (x + 1)


@pytest.mark.parametrize("curve", V.CURVES)
def test_adversarial_set_holds_every_kind(curve):
    """members and non-members of every kind, a torsion point of full order per prime power (asserted inside the makers)"""
    adv, want = V.adversarial(curve), V.membership(curve)
    assert len(adv) == len(want) and 0 < sum(want)
    if curve in V.BLS12:
        assert sum(want) < len(want)
        kinds = {k for k, _ in adv}
        assert {"torsion %d^%d" % f for f in V.FACTORS[curve]} <= kinds and {"G + T", "member", "pure torsion", "raw", "x = 0", "infinity"} <= kinds
    cases, flags = V.on_curve_cases(curve)
    assert 0 < sum(flags) < len(flags)


@pytest.mark.parametrize("curve", V.BLS12)
def test_shortcut_agrees_with_the_definition_over_integers(curve):
    """phi(P) = -[x^2] P with the generator's cube root against r * P = O, on the whole adversarial set, in Python integers alone"""
    p = S.field(curve)[0]
    G = R.generator(curve)
    w = next(pow(g, (p - 1) // 3, p) for g in range(2, 50) if pow(g, (p - 1) // 3, p) != 1)
    betas = [b for b in (w, w * w % p) if V.phi_matches(curve, b, G)]
    assert len(betas) == 1
    for (kind, q), want in zip(V.adversarial(curve), V.membership(curve)):
        got = 1 if q is R.INF or V.phi_matches(curve, betas[0], q) else 0
        assert got == want, (curve, kind, q)


# ---- the generated constants ---------------------------------------------------------------------------------------------------------------

def test_generated_header_is_current():
    want = _gen_constants().render_validate()
    assert open(os.path.join(ROOT, "poly_commit_amd", "csrc", "validate_constants.h")).read() == want, "run tools/gen_constants.py"


@pytest.mark.parametrize("curve", V.BLS12)
def test_generated_beta_is_the_generator_s(curve):
    """the beta' the bodies use satisfies phi(G) = -[x^2] G; the other cube root does not; which of the two glv_constants.h holds"""
    p, r, _ = R.curve_params(curve)
    x, beta, is_glv = V.constants(V.host_probe(), curve)
    assert x == V.bls12_x(curve)
    assert beta != 1 and pow(beta, 3, p) == 1
    G = R.generator(curve)
    assert V.phi_matches(curve, beta, G) and not V.phi_matches(curve, beta * beta % p, G)
    # the eigenvalue on G1 is -x^2: (beta' Gx, Gy) = (r - x^2) G
    assert (beta * G[0] % p, G[1]) == S.mul(curve, (r - x * x) % r, G)
    assert is_glv == (curve == "bls12_377")        # BLS12-381's GLV root has the eigenvalue x^2 - 1: the other one is needed there


# ---- the bodies, host build ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", V.CURVES)
def test_on_curve_body(curve):
    pr = V.host_probe()
    assert V.check_on_curve(pr, pr, curve) == len(V.on_curve_cases(curve)[0])


@pytest.mark.parametrize("curve", V.CURVES)
def test_plain_ladder_body(curve):
    pr = V.host_probe()
    assert len(V.check_subgroup(pr, pr, curve, "pc_probe_validate_ladder")) == len(V.adversarial(curve))


@pytest.mark.parametrize("curve", V.BLS12)
def test_fast_body_agrees_with_the_plain_ladder(curve):
    pr = V.host_probe()
    fast = V.check_subgroup(pr, pr, curve, "pc_probe_validate_fast")
    ladder = V.check_subgroup(pr, pr, curve, "pc_probe_validate_ladder")
    assert np.array_equal(fast, ladder)


def test_fast_body_exists_for_the_bls12_curves_only():
    import ctypes as C
    pr = V.host_probe()
    w, f = np.zeros(16, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    for cid in (1, 2, 4, -1):
        assert pr.raw("pc_probe_validate_fast", C.c_int(cid), C.c_size_t(1), V.P().p32(w), V.P().p32(f)) != 0


def test_g2_bodies():
    pr = V.host_probe()
    kinds, _, _, sub = V.g2_cases()
    assert V.check_g2(pr, pr) == len(kinds) + sum(1 for s in sub if s is not None)


def test_tally_body():
    pr = V.host_probe()
    assert V.check_tally(pr, pr) == 1 + 1 + 64 + 65 + 257 + 257 + 1000 + 1000
