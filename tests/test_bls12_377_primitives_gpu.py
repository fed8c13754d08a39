"""The Fd<P> operations of BLS12-377's two fields and the XYZZ group law of its G1 as compiled for gfx950, one primitive per lane
(tests/hip/probe_field_bls12_377.hip, probe_curve_bls12_377.hip in libpc_probe.so): the case tables of tests/harness/probe.py --
operands at 0, 1, p - 1 and through the lazy range up to 2p -- bit for bit against Python integers (the private copy of the
reference, tests/harness/ref377.py) and word for word against the host build of the same bodies.  tests/test_bls12_377_cpu.py runs
the same cases through the host build alone."""
import pytest

from harness import ref377 as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import poly_commit_amd as pc
    pc.load_library()          # brings torch's bundled HIP runtime up first (see load_library), whichever test file runs first
    return B.probe().device_probe()


@pytest.fixture(scope="module")
def host():
    return B.probe().host_probe()


@pytest.mark.parametrize("group", ["products", "fused", "additive", "inv", "lazy_products", "lazy_fused", "lazy_additive"])
@pytest.mark.parametrize("field", [B.FQ, B.FR])
def test_field(dev, host, field, group):
    assert B.probe().check_field(dev, host, field, group) > 0


@pytest.mark.parametrize("group", ["add_affine", "add", "dbl", "add_affine_lz"])
def test_curve(dev, host, group):
    assert B.probe().check_curve(dev, host, B.CURVE, group) > 0


def test_lazy_flags(dev):
    P = B.probe()
    assert dev.raw("pc_probe_field_lazy_bls12_377", P.C.c_int(0)) == 3 and dev.raw("pc_probe_field_lazy_store_bls12_377", P.C.c_int(0)) == 1
