"""CPU twin of tests/test_device_primitives_gpu.py: the same operand sets and the same Python-integer expectations
(tests/harness/probe.py), run through the host build of the probe bodies (tests/hip, compiled by g++ and looped over lane by lane).
It proves without a GPU that the case tables and the expectations are right, so that a difference on the device can only come from
the device's own code (the product-scanning multiplier of fp32.hpp, the column forms of fp30.hpp, the DPP exchanges of half_add)."""
import pytest

from harness import probe as P


@pytest.fixture(scope="module")
def host():
    return P.host_probe()


@pytest.mark.parametrize("group", P.FIELD_GROUPS)
@pytest.mark.parametrize("field", P.FIELDS)
def test_field(host, field, group):
    P.check_field(host, host, field, group)


@pytest.mark.parametrize("group", P.FQ30_GROUPS)
def test_fq30(host, group):
    assert P.check_fq30(host, host, group) > 0


@pytest.mark.parametrize("group", P.FQ2_GROUPS)
def test_fq2(host, group):
    assert P.check_fq2(host, host, group) > 0


@pytest.mark.parametrize("group", P.CURVE_GROUPS)
@pytest.mark.parametrize("curve", P.GROUPS)
def test_curve(host, curve, group):
    P.check_curve(host, host, curve, group)


def test_chain30(host):
    assert P.check_chain30(host, host) == 13


@pytest.mark.parametrize("curve", P.G1_CURVES)
def test_half_add(host, curve):
    assert P.check_half_add(host, host, curve) == 7 * 32


def test_operand_sets():
    """the sets hold what the multiplier's edge cases need, for every field"""
    for name in P.FIELDS:
        f = P.Field(name)
        c, lz = f.canonical_set(), f.lazy_set()
        assert {0, 1, f.p - 1, f.R % f.p} <= set(c) and all(v < f.p for v in c) and len(c) >= 50
        assert {f.p, 2 * f.p, 2 * f.p - 1} <= set(lz) and max(lz) == 2 * f.p
        assert any(all((v >> (32 * i)) & 0x80000000 for i in range(f.N - 1)) for v in c)      # bit 31 of the low limbs set
    assert [n for n in P.FIELDS if P.Field(n).lazy] == ["bls12_381_fq", "bn254_fq", "bn254_fr"]
