"""The blocking MSM lane that G2 keys and twisted Edwards keys share (csrc/blocking_lane.hpp, key.hpp) on the paths no other test
reaches: pc_hip_ctx_trim over a lane that has run, and the phase brackets a blocking MSM leaves for pc_hip_last_msm_phases_ms.  Three
lanes: a G2 key's, a twisted Edwards key's, and that key's many-MSM pass.  The keys are known multiples k_i of the generator, so the
expected sum of an MSM is one multiplication in tests/harness/g2ref.py / teref.py: (sum_i s_i k_i mod r) * G."""
import math

import numpy as np
import pytest

from harness import g2ref as G
from harness import teref as E

pytestmark = pytest.mark.gpu
N = 1000
M, B = 33, 4      # the many-MSM pass: 4 MSMs of 33 pairs


def key_scalars(n):
    return [(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % E.R for i in range(n)]


def rand_scalars(seed, n, r):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % r for _ in range(n)]


@pytest.fixture(scope="module")
def own_ctx():
    """a context of its own: the tests trim it and switch its timing"""
    import poly_commit_amd as pc
    c = pc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g2_case(own_ctx):
    """(key, scalars, expected point): 1000 G2 points"""
    ks = [k % G.R for k in key_scalars(N)]
    key = own_ctx.upload_g2_srs("bls12_381", G.points_array(G.fixed_base(G.generator()).mul_many(ks)))
    s = rand_scalars(11, N, G.R)
    yield key, G.scalars_array(s, False), G.mul(sum(a * b for a, b in zip(s, ks)) % G.R, G.generator())
    key.free()


@pytest.fixture(scope="module")
def te_case(own_ctx):
    """(key, scalars, expected point, rows of the many-MSM pass, their expected points): 1000 ed_on_bls12_381 points"""
    ks = key_scalars(N)
    key = own_ctx.upload_te_srs("ed_on_bls12_381", E.points_array(E.fixed_base(E.GEN).mul_many(ks)))
    s = rand_scalars(12, N, E.R)
    rows = [rand_scalars(20 + j, M, E.R) for j in range(B)]
    wants = [E.mul(sum(a * b for a, b in zip(r, ks)) % E.R, E.GEN) for r in rows]
    rows_arr = E.scalars_array([k for r in rows for k in r], False).reshape(B, M, 32)
    yield key, E.scalars_array(s, False), E.mul(sum(a * b for a, b in zip(s, ks)) % E.R, E.GEN), rows_arr, wants
    key.free()


def run_trim_run(ctx, key, run, decode, want):
    first = run()
    assert decode(first) == want
    before = key.bytes_resident()["lanes"]
    assert before > 0
    ctx.trim()
    assert key.bytes_resident()["lanes"] <= before
    second = run()
    assert second.tobytes() == first.tobytes()
    assert decode(second) == want
    assert key.bytes_resident()["lanes"] > 0


def test_trim_keeps_a_blocking_lane_usable(own_ctx, g2_case, te_case):
    """one MSM, Context.trim(), the same MSM: the same bytes, the reference's point, and a lane that is not larger after the trim"""
    own_ctx.set_timing(False)
    g2_key, g2_s, g2_want = g2_case
    run_trim_run(own_ctx, g2_key, lambda: g2_key.msm(g2_s)[0], lambda out: G.point_from_bytes(out.tobytes()), g2_want)
    te_key, te_s, te_want, rows, row_wants = te_case
    run_trim_run(own_ctx, te_key, lambda: te_key.msm(te_s)[0], lambda out: E.point_from_bytes(out.tobytes()), te_want)
    # the many-MSM lane is the key's second pipeline: the single MSM above made the first, so "lanes" counts both
    run_trim_run(own_ctx, te_key, lambda: te_key.msm_many(rows)[0], lambda out: [E.point_from_bytes(o.tobytes()) for o in out], row_wants)


def assert_brackets(phases):
    assert len(phases) == 8 and all(math.isfinite(p) and p >= 0 for p in phases), phases
    assert any(p > 0 for p in phases), phases


def test_phases_after_a_blocking_msm(own_ctx, g2_case, te_case):
    """with timing on every blocking MSM leaves its brackets where last_msm_phases_ms reads them; with timing off they are all 0"""
    g2_key, g2_s, g2_want = g2_case
    te_key, te_s, te_want, rows, row_wants = te_case
    own_ctx.set_timing(True)
    try:
        assert E.point_from_bytes(te_key.msm(te_s)[0].tobytes()) == te_want
        assert_brackets(own_ctx.last_msm_phases_ms())
        assert [E.point_from_bytes(o.tobytes()) for o in te_key.msm_many(rows)[0]] == row_wants
        assert_brackets(own_ctx.last_msm_phases_ms())
        assert G.point_from_bytes(g2_key.msm(g2_s)[0].tobytes()) == g2_want
        assert_brackets(own_ctx.last_msm_phases_ms())
        out, inf = g2_key.msm(np.zeros((0, 32), dtype=np.uint8))      # the empty sum plans nothing and must not fail
        assert inf and G.point_from_bytes(out.tobytes()) is G.INF
    finally:
        own_ctx.set_timing(False)
    assert E.point_from_bytes(te_key.msm(te_s)[0].tobytes()) == te_want
    assert own_ctx.last_msm_phases_ms() == [0.0] * 8
