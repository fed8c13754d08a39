"""The Fd<P> operations of ed_on_bls12_381's two fields and the twisted Edwards code of csrc/te.hpp as compiled for gfx950
(tests/hip/probe_field_te.hip, probe_te.hip in libpc_probe.so): one primitive per lane on boundary operands and arbitrary
representatives, chains on a running sum with neighbouring lanes diverging, and the product's own kernel bodies -- the two folds at
the NAF boundaries, TeBatchAffineBody at ragged run lengths, TeDblRowBody through the low-order chain, the subgroup flags, derive and
strip.  The case tables are those of tests/test_te_primitives_cpu.py (tests/harness/teprobe.py): bit for bit against
tests/harness/teref.py and Python integers AND word for word against the host build of the same units.  Every launch is at most a
few thousand lanes; a non-zero HIP status of a probe entry point fails the test with the status in the message, and nothing more is
launched after one."""
import pytest

from harness import teprobe as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import poly_commit_amd as pc
    pc.load_library()          # brings torch's bundled HIP runtime up first (see load_library), whichever test file runs first
    return T.device_probe()


@pytest.fixture(scope="module")
def host():
    return T.host_probe()


@pytest.mark.parametrize("group", sorted(T.FIELD_LANES) + sorted(T.FIELD_LANES_LAZY))
@pytest.mark.parametrize("field", [T.FQ, T.FR])
def test_field(dev, host, field, group):
    want = T.FIELD_LANES[group] if group in T.FIELD_LANES else (T.FIELD_LANES_LAZY[group] if field == T.FR else 0)
    assert T.check_field(dev, host, field, group) == want


def test_lazy_flags(dev):
    assert T.lazy_flags(dev) == [(0, 0), (3, 1)]


def test_add_affine(dev, host):
    assert T.check_madd(dev, host) == 81 * 17


def test_add(dev, host):
    assert T.check_add(dev, host) == 81 * 81


def test_dbl_to_affine_from_affine_derive_neg(dev, host):
    assert T.check_unary(dev, host) == 2 * 81 + 3 * 17


def test_chain(dev, host):
    """every index list in ONE launch, one lane each: neighbouring lanes double, cancel, stay empty and add at the same time"""
    assert T.check_chain(dev, host) == 16


def test_batch_affine(dev, host):
    assert T.check_batch_affine(dev, host) == 3 * (1 + 1 + 15 + 16 + 17 + 33 + 40)


def test_fold_table_row_step(dev, host):
    assert T.check_row_step(dev, host) == 252 * 24


def test_fold_digits(dev):
    assert T.check_fold_digits(dev) == 12


def test_folds(dev, host):
    assert T.check_folds(dev, host) == 12 * 2 * 24


def test_subgroup_flags(dev, host):
    assert T.check_subgroup(dev, host) == 22


def test_derive_strip(dev, host):
    assert T.check_derive_strip(dev, host) == 2 * 17
