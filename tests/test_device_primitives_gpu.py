"""The field and curve primitives of csrc/ as compiled for gfx950, one primitive per lane (tests/hip/libpc_probe.so, built by
poly_commit_amd/build.py), on the boundary operands of every operand class: bit for bit against Python integers AND word for word
against the host build of the same probe bodies.  The cases and expectations are those of tests/test_device_primitives_cpu.py
(tests/harness/probe.py).  Each test is a few launches of at most a few ten thousand lanes; a non-zero HIP status of a probe entry
point fails the test with the status in the message, and nothing is retried."""
import pytest

from harness import probe as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return P.device_probe()


@pytest.fixture(scope="module")
def host():
    return P.host_probe()


@pytest.mark.parametrize("group", P.FIELD_GROUPS)
@pytest.mark.parametrize("field", P.FIELDS)
def test_field(dev, host, field, group):
    P.check_field(dev, host, field, group)


@pytest.mark.parametrize("group", P.FQ30_GROUPS)
def test_fq30(dev, host, group):
    assert P.check_fq30(dev, host, group) > 0


@pytest.mark.parametrize("group", P.FQ2_GROUPS)
def test_fq2(dev, host, group):
    assert P.check_fq2(dev, host, group) > 0


@pytest.mark.parametrize("group", P.CURVE_GROUPS)
@pytest.mark.parametrize("curve", P.GROUPS)
def test_curve(dev, host, curve, group):
    P.check_curve(dev, host, curve, group)


def test_chain30(dev, host):
    """every index list in ONE launch, one lane each: neighbouring lanes double, cancel, meet infinity and add at the same time"""
    assert P.check_chain30(dev, host) == 13


@pytest.mark.parametrize("curve", P.G1_CURVES)
def test_half_add(dev, host, curve):
    """the lane pairs of a wave take every branch of half_add side by side (DPP exchanges under divergence), then one wave per kind"""
    assert P.check_half_add(dev, host, curve) == 7 * 32
