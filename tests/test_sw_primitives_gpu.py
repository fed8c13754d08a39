"""The pieces of sample_generators over the short Weierstrass curves as compiled for gfx950 (csrc/sw_setup.hpp through
tests/hip/probe_sw_setup.hip), one operand per lane, all four base fields: the square root, from_random_bytes on crafted digests, the
cofactor multiplication and the per-index body -- the case tables of tests/harness/swsetupprobe.py against Python integers AND word for
word against the host build.  Every launch is at most a few hundred lanes."""
import pytest

from harness import swsetupprobe as P

pytestmark = pytest.mark.gpu
CURVES = P.CURVES


@pytest.fixture(scope="module")
def dev():
    import poly_commit_amd as pc
    pc.load_library()          # brings torch's bundled HIP runtime up first, whichever test file runs first
    return P.device_probe()


@pytest.fixture(scope="module")
def host():
    return P.host_probe()


@pytest.mark.parametrize("curve", CURVES)
def test_sqrt(dev, host, curve):
    """0, 1, 4, p - 1, a non-residue, the generator's x^3 + b, SQRT_C, SQRT_C^2 and SQRT_C^(2^(S-1)) for the two-adic fields, 64 seeded
    squares and 64 seeded non-squares"""
    assert P.check_sqrt(dev, host, curve) == P.sqrt_lanes(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_from_random_bytes(dev, host, curve):
    """all-zero with and without 0x40 in byte 31, all-0xff, x = p - 1, p, p + 1 under the mask, the four flag combinations on an x whose
    computed root is the smaller and on one whose computed root is the larger, bit 255, and the digests indices 0..15 consume"""
    assert P.check_try(dev, host, curve) == P.try_lanes(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_cofactor(dev, host, curve):
    """the identity, the generator, seeded points outside the subgroup, and points of the cofactor torsion (r * P)"""
    assert P.check_cofactor(dev, host, curve) == P.cofactor_lanes(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_sample_body(dev, host, curve):
    assert P.check_sample(dev, host, curve) == 64 + 2
