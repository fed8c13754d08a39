"""GPU: the bucket accumulation with its prefetched base staged in the workgroup's LDS tile (csrc/msm_coop.hpp StageLds, the BLS12-381
radix-2^30 kernel).  BLS12-381 G1 MSMs through pc_hip_msm on a key whose window table is precomputed -- the path bench.py runs --
every result against the oracle (O.msm_pippenger, and O.msm_naive up to 256 pairs).  The shapes are the smallest at which the staging
can go wrong: a one-entry chunk (the prefetch index clamps), a last chunk shorter than the others, a partly filled last workgroup
(lanes that run no loop but share the tile), buckets that span many lanes (the in-workgroup scan reuses the tile right behind the
loop), infinity / doubling / cancellation among the staged bases, negative digits, and repeated calls on one key (stale tile
contents, workspace growth)."""
import numpy as np
import pytest

import oracle_lib as O
import pyref as R

pytestmark = pytest.mark.gpu

CURVE = "bls12_381"
NMAX = 40000
SIZES = (1, 2, 63, 64, 65, 257, 4099, 40000)
_state = {}


@pytest.fixture(scope="module")
def key(ctx):
    """One key for the whole file: NMAX bases with the special ones below, its window table built for every call length."""
    bases = O.gen_bases(CURVE, NMAX)
    pts = O.array_to_points(CURVE, bases[:64])
    # the point at infinity at the key's first base, around multiples of 16 and at the last base of the 4099-pair calls.  Where these land
    # inside a chunk depends on the call's chunk length and on the sorted order, which the library chooses: the indices are spread so that
    # chunk edges are likely to be hit (with equal scalars a bucket's entries keep the base order), not placed.  The exact first / middle /
    # last positions of a chunk are set by tests/test_acc_stage_cpu.py, which controls the entry list
    for j in (0, 7, 15, 16, 31, 32, 100, 4098):
        bases[j] = 0
    bases[3] = bases[2]                                  # a base twice (equal digits: the doubling path)
    bases[49] = bases[48]
    bases[5] = O.points_to_array(CURVE, [R.ec_neg(CURVE, pts[4])])[0]      # a base and its negative (equal digits: sum to infinity)
    bases[41] = O.points_to_array(CURVE, [R.ec_neg(CURVE, pts[40])])[0]
    srs = ctx.upload_srs(CURVE, bases)
    srs.precompute(min_pairs=1)
    yield srs, bases
    srs.free()


def want(bases, off, scalars):
    k = (off, len(scalars), scalars.tobytes())
    if k not in _state:                                   # one oracle run per distinct input, shared by the tests below
        b = np.ascontiguousarray(bases[off:])
        w = O.msm_pippenger(CURVE, b, scalars, 8, 1)
        if len(scalars) <= 256:
            assert (w == O.msm_naive(CURVE, b, scalars)).all()
        _state[k] = w
    return _state[k]


def check(srs, bases, scalars, off=0):
    scalars = np.ascontiguousarray(scalars)
    got, inf = srs.msm(scalars, base_offset=off) if off else srs.msm(scalars)
    w = want(bases, off, scalars)
    assert (got == w).all(), (len(scalars), off)
    assert inf == (not w.any())


@pytest.mark.parametrize("n", SIZES)
def test_uniform_scalars(key, n):
    srs, bases = key
    check(srs, bases, O.gen_scalars(CURVE, 0xACC0 + n, n))


@pytest.mark.parametrize("n", SIZES)
def test_all_scalars_equal_one_bucket_spans_many_lanes(key, n):
    """Every scalar the same: each window's digits fall into one bucket, whose run spans all the lanes (transparent lanes: the scan
    puts points into the tile right behind the loop that staged bases in it).  The special bases sit inside those runs."""
    srs, bases = key
    check(srs, bases, np.repeat(O.gen_scalars(CURVE, 0x5A3E, 1), n, axis=0))


def test_doubling_and_cancellation_at_the_start_of_a_run(key):
    srs, bases = key
    one = O.ints_to_limbs([1, 1], 4)
    k = np.repeat(O.gen_scalars(CURVE, 0xD0B1, 1), 2, axis=0)
    for sc in (one, k):
        check(srs, bases, sc, off=2)                      # P, P: the second addition doubles
        check(srs, bases, sc, off=48)
        check(srs, bases, sc, off=4)                      # P, -P: infinity
        check(srs, bases, sc, off=40)
        check(srs, bases, sc, off=15)                     # infinity, infinity
        check(srs, bases, sc, off=6)                      # P, infinity


@pytest.mark.parametrize("n", (65, 4099))
def test_all_digits_negative(key, n):
    srs, bases = key
    r = R.FIELDS["bls12_381_fr"]["p"]
    check(srs, bases, O.ints_to_limbs([r - 1 - i for i in range(n)], 4))


def test_repeated_calls_on_one_key(key):
    """The same call twice in one process, and once more after a larger call on the same key."""
    srs, bases = key
    small = O.gen_scalars(CURVE, 0xACC0 + 257, 257)
    large = O.gen_scalars(CURVE, 0xACC0 + 40000, 40000)
    check(srs, bases, small)
    check(srs, bases, small)
    check(srs, bases, large)
    check(srs, bases, small)
    check(srs, bases, large)
