"""The MSM's bucket reduction on the device, directly: HipBackend::bucket_level -- the serial BucketLevelBody, k_bucket_level_coop and the
two-lane k_bucket_level_coop2 of csrc/msm_coop.hpp, kernels that run nowhere but on the card -- through the test-only probe
(tests/hip/probe_reduce.hip) against the contract restated in tests/harness/reduceref.py.

Levels alone: every (K, mode, weight_off, n_old) that msm_plan_levels yields over the sweep of reduceref.sweep_calls (table-free
c = 2 .. 20 at 5000 and 2^20 pairs, the window table plain and GLV, many-MSM shapes, G2) and the fixed edges, each with every bucket
content of reduceref.CONTENTS and one-hot exhaustively, cnt = 1 and 3.  Every output point is held against (sum of integer logarithms
mod r) G, never against another bucket method; the cnt points behind the last array must keep the probe's 0xff preset; on G1 the words
of the one-lane and the two-lane kernel are compared for every K <= 128 (msm_coop.hpp: "same intermediate values as XyzzD::add").
Whole plans on given buckets: every level of the production plan chained in reduce_and_download's layout, checked through
sum_a 2^arr_exp[a] out_a[w] = sum_j (j + 1) B[w][j], SubFoldBody's result included in many-MSM mode, also under the knobs the
environment variables reach.  Whole MSMs through the C ABI with every bucket full: one pair per (window, bucket), so the accumulation
is trivial and the reduction is what runs.  Every comparison is exact; mode 2 does not exist on G2, nothing else is left out."""
import ctypes as C
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from harness import g2ref as G2
from harness import probe as P
from harness import reduceref as RR
from harness import signedkey as SK
from harness import sortref as S
from harness import teref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = list(RR.GROUPS)
G1 = list(RR.G1)


@functools.lru_cache(None)
def dev():
    import poly_commit_amd as pc
    pc.load_library()          # brings torch's bundled HIP runtime up first (see load_library), whichever test file runs first
    return P.device_probe()


# ---- levels alone ------------------------------------------------------------------------------------------------------------------------

def level_on_device(g, K, mode, woff, n_old):
    """one tuple: every content at cnt = 1 and 3, then one-hot at cnt = K; -> points checked"""
    what = "%s K=%d mode=%d weight_off=%d n_old=%d" % (g.name, K, mode, woff, n_old)
    twin = None if (mode == 0 or K > 128 or g.g2) else 3 - mode       # the other cooperative kernel: same words
    n = 0
    for name in RR.contents_for(g):
        for cnt in (1, 3):
            xw, ow, xl, ol = RR.level_case(g, name, K, cnt, n_old, 11 * K + n_old)
            out = RR.run_level(dev(), g, K, woff, cnt, n_old, mode, xw, ow)
            n += RR.check_level(g, out, RR.expected_level(g.r, K, woff, n_old, mode, xl, ol), "%s %s cnt=%d" % (what, name, cnt))
            if twin:
                other = RR.run_level(dev(), g, K, woff, cnt, n_old, twin, xw, ow)
                assert (other == out).all(), "%s %s cnt=%d: the words of mode 1 and mode 2 differ" % (what, name, cnt)
            if mode == 0:          # the same body on both sides: the same words
                assert (RR.run_level(P.host_probe(), g, K, woff, cnt, n_old, 0, xw, ow) == out).all(), "%s %s: device and host words differ" % (what, name)
    xw, ow, _, _ = RR.one_hot_case(g, K, n_old, K + n_old)
    out = RR.run_level(dev(), g, K, woff, K, n_old, mode, xw, ow)
    n += RR.check_one_hot(g, out, K, woff, n_old, mode, xw, ow, what)
    if twin:
        assert (RR.run_level(dev(), g, K, woff, K, n_old, twin, xw, ow) == out).all(), "%s one-hot: the words of mode 1 and mode 2 differ" % what
    return n


LEVEL_PARAMS = [(grp, mode, woff) for grp in GROUPS for mode in (0, 1, 2) for woff in (0, 1) if not (grp.endswith("_g2") and mode == 2)]


@pytest.mark.parametrize("group,mode,weight_off", LEVEL_PARAMS)
def test_levels_alone(group, mode, weight_off):
    """every tuple of the sweep and of the fixed edges with this mode and weight_off, on this group"""
    g = RR.Group(group)
    tuples = [t for t in RR.level_tuples(dev(), g) if t[1] == mode and t[2] == weight_off]
    assert tuples, "the sweep yields no such level"
    t0, n = time.time(), 0
    for K, _, _, n_old in tuples:
        n += level_on_device(g, K, mode, weight_off, n_old)
    print("%s mode %d weight_off %d: %d tuples, %d points, %.1f s" % (group, mode, weight_off, len(tuples), n, time.time() - t0))


def test_the_sweep_reaches_every_kind_of_level():
    """the tuple list holds what the planner makes: serial levels with one and with several older arrays, both cooperative kernels
    at the first level and behind serial ones, n_old up to 14"""
    t = set(RR.level_tuples(dev(), RR.Group("bls12_381")))
    assert {(8, 0, 1, 0), (8, 0, 0, 1), (16, 2, 1, 0), (256, 1, 1, 0), (256, 1, 0, 1), (128, 1, 0, 2), (64, 2, 0, 9), (16, 2, 0, 13)} <= t
    assert set(RR.SERIAL_EDGES) <= t and set(RR.COOP_EDGES) <= t
    t2 = RR.level_tuples(dev(), RR.Group("bls12_381_g2"))
    assert all(mode != 2 and K <= 128 for K, mode, _, _ in t2) and any(mode == 1 and n_old >= 6 for _, mode, _, n_old in t2)


# ---- whole plans on given buckets ------------------------------------------------------------------------------------------------------

KNOBS = ({"K0": 4}, {"coop2_max_points": 0}, {"coop_max_points": 1 << 30})
WHOLE_CONTENTS = ("random", "equal_other_words", "alternating")


def whole_calls(g):
    """(n, c, tbl, glv, subs, knobs).  W = 3 is what the many-MSM mode with three rows gives (the table-free W is the digit count);
    G2 is table-free only and runs with the W its width gives"""
    calls = [(5000, c, 0, 0, 0, {}) for c in range(2, 14)]
    if g.g2:
        return calls + [(5000, c, 0, 0, 0, k) for c in (4, 9, 13) for k in KNOBS]
    calls += [(3 * 1024, c, 1, 0, 3, {}) for c in range(2, 14)]
    calls += [(5000, c, 1, glv, 0, {}) for c in (13, 16) for glv in (0, 1)]
    calls += [(4 * 1024, 11, 1, 0, 4, {}), (8 * 1024, 8, 1, 1, 8, {})]                       # many-MSM plans: SubFoldBody runs
    calls += [call[:5] + (k,) for call in ((5000, 5, 0, 0, 0), (5000, 9, 0, 0, 0), (5000, 12, 0, 0, 0), (5000, 13, 0, 0, 0), (3 * 1024, 12, 1, 0, 3),
                                           (5000, 16, 1, 0, 0)) for k in KNOBS]
    return calls


def large_calls(g):
    """one bucket set of 2^13 .. 2^19 points: the window table's plans, short calls (two-lane levels) and long ones (none)"""
    n = 1 << 20 if g.name == "bls12_381" else 5000
    return [(n, c, 1, 0, 0, {}) for c in range(14, 21)] + [(n, 20, 1, 1, 0, {})] + [(5000, 20, 1, 0, 0, k) for k in KNOBS]


@pytest.mark.parametrize("content", WHOLE_CONTENTS)
@pytest.mark.parametrize("group", GROUPS)
def test_whole_plans_on_given_buckets(group, content):
    g = RR.Group(group)
    t0, n = time.time(), 0
    for i, call in enumerate(whole_calls(g)):
        n += RR.run_whole(dev(), g, call, content, 100 + i)
    print("%s %s: %d plans, %d bucket sets, %.1f s" % (group, content, len(whole_calls(g)), n, time.time() - t0))


@pytest.mark.parametrize("content", WHOLE_CONTENTS)
@pytest.mark.parametrize("group", ["bls12_381", "bn254"])
def test_whole_plans_of_one_large_bucket_set(group, content):
    """c = 14 .. 20 over the window table, on one 12-limb and one 8-limb curve"""
    g = RR.Group(group)
    t0 = time.time()
    for i, call in enumerate(large_calls(g)):
        RR.run_whole(dev(), g, call, content, 200 + i)
    print("%s %s: %d plans, %.1f s" % (group, content, len(large_calls(g)), time.time() - t0))


@pytest.mark.parametrize("group", GROUPS)
def test_whole_plans_one_hot(group):
    """c <= 8: every bucket is once the only finite one of its set"""
    g = RR.Group(group)
    for c in range(2, 9):
        call = (5000, c, 0, 0, 0, {}) if g.g2 else (1024 << (c - 1), c, 1, 0, 1 << (c - 1), {})      # G1: as many rows as buckets
        assert RR.run_whole_one_hot(dev(), g, call, c) >= 1 << (c - 1)
        if not g.g2:
            assert RR.run_whole_one_hot(dev(), g, (5000, c, 0, 0, 0, {}), c) >= 1 << (c - 1)


# ---- whole MSMs through the C ABI with every bucket full -------------------------------------------------------------------------------

KEYS = {"one_base": SK.one_base, "signed": SK.signed, "signed_holes": lambda curve, n: SK.signed(curve, n, holes=True), "unsigned": SK.unsigned}


def _is(got, want, what):
    out, inf = got
    assert (out == want).all(), what
    assert bool(inf) == (not want.any()), what


@pytest.mark.parametrize("c", [2, 3, 4, 5, 9, 12, 14])
@pytest.mark.parametrize("curve", G1)
def test_whole_msm_with_every_bucket_full(ctx, curve, c):
    """set_msm_tuning(c, 0), one pair per (window, bucket); all buckets equal, neighbours P and -P, the same with holes, unsigned"""
    g = RR.Group(curve)
    sc = RR.full_bucket_scalars(g.r, g.bits, c)
    limbs = SK.limbs(sc)
    ctx.set_msm_tuning(c, 0)
    try:
        for name, make in KEYS.items():
            key = make(curve, len(sc))
            srs = ctx.upload_srs(curve, key.bases)
            try:
                _is(srs.msm(limbs), SK.expected(key, sc), (curve, c, name))
                shape = ctx.last_msm_shape()
                assert shape["window_bits"] == c and not shape["window_table"] and shape["buckets"] == (g.bits // c + 1) << (c - 1)
            finally:
                srs.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("glv", [False, True])
@pytest.mark.parametrize("curve", G1)
def test_whole_msm_over_a_13_bit_table_with_every_bucket_full(ctx, curve, glv):
    """plain: the layout's pairs land in ONE bucket set, every bucket holding one base per window.  GLV: scalars a + lambda b with a
    and b of the layout, so that both halves' sets are full; the device's split is taken from sortref and the fullness asserted"""
    c, g = 13, RR.Group(curve)
    if glv:
        a = RR.full_bucket_scalars(g.r, S.HALF_BITS, c, limit=1 << 120)
        lam = S.glv(curve)["lam"]
        sc = [(x + lam * a[(i + 7) % len(a)]) % g.r for i, x in enumerate(a)]
    else:
        sc = RR.full_bucket_scalars(g.r, g.bits, c)
    n = len(sc)
    geom = S.Geom(curve, n, c, tbl_stride=n, glv=int(glv))
    keys, _ = S.ref_sort(geom, S.to_limbs(sc))
    assert (np.bincount(keys, minlength=geom.NB) > 0).all() and geom.NB == (2 if glv else 1) << (c - 1), "a bucket is empty"
    limbs = SK.limbs(sc)
    for name, make in KEYS.items():
        key = make(curve, n)
        srs = ctx.upload_srs(curve, key.bases)
        try:
            srs.precompute(window_bits=c, min_pairs=1, glv=glv)
            _is(srs.msm(limbs), SK.expected(key, sc), (curve, glv, name))
            shape = ctx.last_msm_shape()
            assert shape["window_bits"] == c and shape["window_table"] and shape["buckets"] == geom.NB
        finally:
            srs.free()


def _pattern_logs(name, n, ks, r):
    """signedkey's key kinds as logarithms over another group's pool ks"""
    j = np.arange(n)
    idx = {"one_base": np.zeros(n, dtype=np.intp), "unsigned": (j // 2) % SK.POOL}.get(name)
    if idx is None:
        idx = (j // 2) % SK.POOL + SK.POOL * (j & 1)
        if name == "signed_holes":
            idx[j % SK.HOLE_PERIOD == SK.HOLE_AT] = 2 * SK.POOL
    table = list(ks) + [r - k for k in ks] + [0]
    return idx, [table[i] for i in idx]


@pytest.mark.parametrize("c", [4, 7, 10])
def test_whole_g2_msm_with_every_bucket_full(ctx, c):
    g = RR.Group("bls12_381_g2")
    sc = RR.full_bucket_scalars(g.r, g.bits, c)
    pool = G2.points_array([g.mul_g(e) for e in g.pool_logs()])
    arr = G2.scalars_array(sc, False)
    ctx.set_msm_tuning(c, 0)
    try:
        for name in KEYS:
            idx, logs = _pattern_logs(name, len(sc), g.ks, g.r)
            want = g.mul_g(sum(s * e for s, e in zip(sc, logs)))
            k = ctx.upload_g2_srs("bls12_381", np.ascontiguousarray(pool[idx]))
            try:
                out, inf = k.msm(arr)
                assert G2.point_from_bytes(out.tobytes()) == want and inf == (want is G2.INF), (c, name)
                assert ctx.last_msm_shape()["window_bits"] == c
            finally:
                k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


def test_whole_te_msm_with_every_bucket_full(ctx):
    """pc_hip_te_msm at the width it picks for a call of 2^13 pairs: the layout of that width, filled up with zero scalars"""
    n = 1 << 13
    c = RR.choose_c(n, 252)
    sc = RR.full_bucket_scalars(E.R, 252, c)
    assert c == 9 and len(sc) <= n
    sc = sc + [0] * (n - len(sc))
    rnd = np.random.RandomState(0x7E)
    ks = [int.from_bytes(rnd.bytes(31), "little") % E.R | 1 for _ in range(SK.POOL)]
    pts = E.fixed_base(E.GEN).mul_many(ks)
    pool = E.points_array(pts + [E.neg(p) for p in pts] + [E.IDENT])
    arr = E.scalars_array(sc, False)
    for name in KEYS:
        idx, logs = _pattern_logs(name, n, ks, E.R)
        t = sum(s * e for s, e in zip(sc, logs)) % E.R
        want = E.fixed_base(E.GEN).mul_many([t])[0] if t else E.IDENT
        k = ctx.upload_te_srs("ed_on_bls12_381", np.ascontiguousarray(pool[idx]))
        try:
            out, ident = k.msm(arr)
            assert E.point_from_bytes(out.tobytes()) == want and ident == (want == E.IDENT), name
            assert ctx.last_msm_shape()["window_bits"] == c
        finally:
            k.free()


CHILD = r'''
import sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
from harness import reduceref as RR
from harness import signedkey as SK
import poly_commit_amd as pc
ctx = pc.Context(0)
for curve in ("bls12_381", "bn254"):
    g = RR.Group(curve)
    for c in (9, 12, 14):
        sc = RR.full_bucket_scalars(g.r, g.bits, c)
        limbs = SK.limbs(sc)
        ctx.set_msm_tuning(c, 0)
        for make in (SK.one_base, SK.signed, SK.unsigned):
            key = make(curve, len(sc))
            srs = ctx.upload_srs(curve, key.bases)
            out, inf = srs.msm(limbs)
            want = SK.expected(key, sc)
            assert (out == want).all() and bool(inf) == (not want.any()), (curve, c, make.__name__)
            assert ctx.last_msm_shape()["window_bits"] == c
            srs.free()
ctx.close()
print("full buckets ok")
'''


@pytest.mark.parametrize("var,value", [("PC_HIP_COOP2_MAX_LOG2", "-1"), ("PC_HIP_COOP_MAX_LOG2", "30"), ("PC_HIP_K0", "4")])
def test_whole_msms_under_the_planner_knobs(var, value):
    """the c = 9, 12, 14 layouts with no two-lane levels, with cooperative levels from the first level on, and with serial groups of
    four (the library reads the variables once per key: a child process)"""
    env = dict(os.environ, **{var: value})
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "full buckets ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
