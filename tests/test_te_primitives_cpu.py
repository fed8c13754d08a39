"""CPU twin of tests/test_te_primitives_gpu.py: the case tables of tests/harness/teprobe.py -- the Fd<P> operations of the two fields
of ed_on_bls12_381 on boundary operands, the twisted Edwards law of csrc/te.hpp one primitive per lane on arbitrary representatives,
chains on a running sum, and the product's own kernel bodies (the folds, the batch normalisation, the fold-table row step, the
subgroup flags, derive and strip) -- run through the host build of the probe units (tests/hip/probe_field_te.hip, probe_te.hip,
compiled by g++ and looped over lane by lane).  It proves without a GPU that the tables and the expectations (tests/harness/teref.py,
Python integers) are right, so that a difference on the device can only come from the device's own code.  Every check returns its
lane count and the exact number is asserted: a table cannot silently shrink."""
import pytest

from harness import teprobe as T


@pytest.fixture(scope="module")
def host():
    return T.host_probe()


@pytest.mark.parametrize("group", sorted(T.FIELD_LANES) + sorted(T.FIELD_LANES_LAZY))
@pytest.mark.parametrize("field", [T.FQ, T.FR])
def test_field(host, field, group):
    """which = 0 is BLS12-381's Fr (no lazy forms: every lazy operation answers PROBE_UNSUPPORTED), which = 1 the 252-bit scalar field"""
    want = T.FIELD_LANES[group] if group in T.FIELD_LANES else (T.FIELD_LANES_LAZY[group] if field == T.FR else 0)
    assert T.check_field(host, host, field, group) == want


def test_lazy_flags(host):
    assert T.lazy_flags(host) == [(0, 0), (3, 1)]


def test_add_affine(host):
    assert T.check_madd(host, host) == 81 * 17


def test_add(host):
    assert T.check_add(host, host) == 81 * 81


def test_dbl_to_affine_from_affine_derive_neg(host):
    assert T.check_unary(host, host) == 2 * 81 + 3 * 17


def test_chain(host):
    assert T.check_chain(host, host) == 16


def test_batch_affine(host):
    assert T.check_batch_affine(host, host) == 3 * (1 + 1 + 15 + 16 + 17 + 33 + 40)


def test_fold_table_row_step(host):
    assert T.check_row_step(host, host) == 252 * 24


def test_fold_digits(host):
    assert T.check_fold_digits(host) == 12


def test_folds(host):
    assert T.check_folds(host, host) == 12 * 2 * 24


def test_subgroup_flags(host):
    assert T.check_subgroup(host, host) == 22


def test_derive_strip(host):
    assert T.check_derive_strip(host, host) == 2 * 17


def test_tables():
    """the tables hold what the issue's edge cases need"""
    S = T.point_set()
    assert T.E.ZERO in S and T.E.IDENT in S and T.E.T2 in S and T.E.T8 in S and len(T.reps()) == 81
    assert set(T.lambdas()[:4]) == {1, T.Q - 1, (1 << 256) % T.Q, (T.Q - 1) // 2} and len(set(T.lambdas())) == 5
    assert len(T.fold_scalars()) == 12 and len(T.fold_right()) == 24
    names = [n for n, _ in T.chain_lists()]
    assert len(names) == 16 and [i for i, n in enumerate(names) if n.startswith("random")] == [2, 6, 10]
