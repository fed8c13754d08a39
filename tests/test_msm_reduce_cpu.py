"""The bucket reduction's contract (tests/harness/reduceref.py) on the CPU: the host build of tests/hip/probe_reduce.hip steps
BucketLevelBody and BucketLevelBitsBody lane by lane -- what the backends of tests/emu run in place of the cooperative kernels -- and
every output is held against integer logarithms.  Also here: the Python restatement of the level plan against msm_plan_levels over the
whole sweep, the checker against outputs with one property broken each, and the probe's refusals.  tests/test_msm_reduce_gpu.py runs
the full lists on the device; the lists here are trimmed to what the CPU steps in about a minute."""
import ctypes as C

import numpy as np
import pytest

from harness import probe as P
from harness import reduceref as RR

GROUPS = list(RR.GROUPS)
KNOB_SETS = ({}, {"K0": 4}, {"coop2_max_points": 0}, {"coop_max_points": 1 << 30}, {"tbl_K0": 16, "K1": 64}, {"coop2_max_entries": 1 << 30})


def host():
    return P.host_probe()


@pytest.mark.parametrize("group", GROUPS)
def test_fixed_base_table_equals_the_reference_scalar_multiplication(group):
    """the table that turns a logarithm into the expected point, against the reference's own double-and-add"""
    g = RR.Group(group)
    for t in (1, 2, 255, 256, g.r - 1, g.ks[0], g.r - g.ks[3], (g.ks[1] * 77 + g.ks[2]) % g.r):
        assert g.mul_g(t) == g.mul_g_slow(t)
    assert g.mul_g(0) is None and g.mul_g(g.r) is None


@pytest.mark.parametrize("group", GROUPS)
def test_python_plan_equals_msm_plan_levels_over_the_sweep(group):
    """every call the level tests take their tuples from, under the default configuration and under each knob"""
    g = RR.Group(group)
    calls = RR.sweep_calls(g) + [(n, c, 0, 0, 0) for c in (21, 24) for n in (31, 1 << 24)]
    for knobs in KNOB_SETS:
        for call in calls:
            got = RR.probe_plan(host(), g, *call, **knobs)
            assert got != RR.BAD_OP and got.key() == RR.plan(g, *call, **knobs).key(), (group, call, knobs)
            assert got.levels[-1][2] == 1 and len(got.arr_exp) == got.levels[-1][3]


def test_the_issue_table_of_plans():
    """the plans the planner gave when it was restated by hand (K, mode, n_old per level)"""
    g = RR.Group("bls12_381")
    short = lambda pl: [(K, mode, n_old) for K, mode, _, n_old in pl.tuples()]
    want = {5: [(16, 2, 0)], 9: [(16, 2, 0), (16, 2, 5)], 12: [(64, 1, 0), (32, 2, 7)], 14: [(8, 0, 0), (32, 1, 1), (32, 2, 6)],
            17: [(8, 0, 0), (128, 1, 1), (64, 2, 8)], 20: [(8, 0, 0), (8, 0, 1), (128, 1, 2), (64, 2, 9)]}
    for c, levels in want.items():
        assert short(RR.plan(g, 5000, c)) == levels, c
    assert short(RR.plan(g, 1 << 20, 9)) == [(256, 1, 0)]
    assert all(mode != 2 for c in range(2, 21) for _, mode, _ in short(RR.plan(g, 1 << 20, c)))
    # over the window table (calls short enough for two-lane levels)
    assert [(K, mode) for K, mode, _ in short(RR.plan(g, 5000, 16, tbl=1))] == [(32, 2)] * 3
    assert short(RR.plan(g, 5000, 16, tbl=1, glv=1)) == [(256, 1, 0), (128, 2, 9)]
    assert short(RR.plan(g, 5000, 20, tbl=1)) == [(8, 0, 0), (256, 1, 1), (16, 2, 9), (16, 2, 13)]
    p23 = RR.plan(g, 5000, 23, tbl=1)
    assert len(p23.levels) == 5 and max(n_old for _, _, n_old in short(p23)) == 14


def cpu_tuples(g):
    """every serial tuple; the cooperative tuples the lane-serial body steps quickly (it is one body for modes 1 and 2)"""
    return [t for t in RR.level_tuples(host(), g) if t[1] == 0 or (t[0] <= 32 and t[3] <= 6) or (t[0] == 256 and t[3] <= 1)]


@pytest.mark.parametrize("group", GROUPS)
def test_levels_alone_on_the_host_build(group):
    g = RR.Group(group)
    n = 0
    for K, mode, woff, n_old in cpu_tuples(g):
        what = "%s K=%d mode=%d weight_off=%d n_old=%d" % (group, K, mode, woff, n_old)
        for name in RR.contents_for(g):
            for cnt in (1, 3):
                xw, ow, xl, ol = RR.level_case(g, name, K, cnt, n_old, 11 * K + n_old)
                out = RR.run_level(host(), g, K, woff, cnt, n_old, mode, xw, ow)
                n += RR.check_level(g, out, RR.expected_level(g.r, K, woff, n_old, mode, xl, ol), "%s %s cnt=%d" % (what, name, cnt))
        if K <= 64:
            xw, ow, _, _ = RR.one_hot_case(g, K, n_old, K + n_old)
            n += RR.check_one_hot(g, RR.run_level(host(), g, K, woff, K, n_old, mode, xw, ow), K, woff, n_old, mode, xw, ow, what)
    assert n > 1000


def whole_calls(g):
    if g.g2:
        return [(5000, c, 0, 0, 0, {}) for c in (2, 5, 8)] + [(5000, 7, 0, 0, 0, {"K0": 4})]
    calls = [(5000, c, 0, 0, 0, {}) for c in (2, 5, 9)] + [(3 * 64, c, 1, 0, 3, {}) for c in (3, 12)]
    if g.name in ("bls12_381", "bn254"):
        calls += [(5000, 14, 1, 0, 0, {}), (1 << 20, 13, 1, 1, 0, {}), (8 * 64, 8, 1, 1, 8, {})]
        calls += [(5000, 12, 0, 0, 0, k) for k in ({"K0": 4}, {"coop2_max_points": 0}, {"coop_max_points": 1 << 30})]
    return calls


@pytest.mark.parametrize("group", GROUPS)
def test_whole_plans_on_given_buckets_on_the_host_build(group):
    g = RR.Group(group)
    for i, call in enumerate(whole_calls(g)):
        for name in ("random", "equal_other_words", "alternating"):
            assert RR.run_whole(host(), g, call, name, 100 + i) > 0
    assert RR.run_whole_one_hot(host(), g, (5000, 4, 0, 0, 0, {}), 5) >= 8


def test_checker_catches_outputs_with_one_property_broken():
    """an output array swapped with its neighbour, the S copy missing, an older-array sum lacking its last element (levels); one
    exponent off by one (whole reduction)"""
    g = RR.Group("bn254")
    K, woff, cnt, n_old, mode = 16, 1, 3, 2, 1
    xw, ow, xl, ol = RR.level_case(g, "random", K, cnt, n_old, 5)
    want = RR.expected_level(g.r, K, woff, n_old, mode, xl, ol)
    out = RR.run_level(host(), g, K, woff, cnt, n_old, mode, xw, ow)
    RR.check_level(g, out, want, "intact")

    def broken(f):
        o = out.copy()
        f(o)
        with pytest.raises(AssertionError):
            RR.check_level(g, o, want, "broken")

    def swap_neighbours(o): o[[1, 2]] = o[[2, 1]]
    def no_s_copy(o): o[1 + RR.lg(K)] = 0xffffffff
    def s_copy_infinite(o): o[1 + RR.lg(K)] = 0
    def write_behind(o): o[-1, 0, 0] = 0
    for f in (swap_neighbours, no_s_copy, s_copy_infinite, write_behind):
        broken(f)
    # the last older array summed without its last element: what the level would put out for inputs that lack it
    ow2 = ow.reshape(n_old, cnt, K, g.PW).copy()
    ow2[n_old - 1, :, K - 1] = 0
    short = RR.run_level(host(), g, K, woff, cnt, n_old, mode, xw, ow2.reshape(-1, g.PW))
    assert any(ol[n_old - 1][i][K - 1] != 0 for i in range(cnt))
    with pytest.raises(AssertionError):
        RR.check_level(g, short, want, "short sum")
    # the whole reduction with one exponent off by one
    call = (5000, 9, 0, 0, 0, {})
    pl = RR.plan(g, *call[:5])
    idx, rep = RR.content("random", (pl.W, pl.nb_win), 3)
    arrays, _ = RR.run_all(host(), g, pl, *call[:5], RR.gather(g, idx, rep).reshape(-1, g.PW))
    RR.check_all(g, pl, arrays, None, RR.logs_of(g, idx), "intact")
    for a in (0, len(pl.arr_exp) - 1):
        exps = list(pl.arr_exp)
        exps[a] += 1
        with pytest.raises(AssertionError):
            RR.check_all(g, pl, arrays, None, RR.logs_of(g, idx), "exponent", exps)


def test_probe_refuses_what_the_level_kernels_cannot_run():
    """PROBE_BAD_OP, with the output buffer untouched"""
    u = C.c_uint32
    for group in ("bn254", "bls12_381_g2"):
        g = RR.Group(group)
        x = np.zeros((1 << 12, g.PW), dtype=np.uint32)

        def level(K, woff, cnt, n_old, mode, out_points=None):
            out = np.full((64, g.PW), 7, dtype=np.uint32)
            st = host().raw("pc_probe_reduce_level", g.id, u(K), u(woff), u(cnt), u(n_old), C.c_int(mode), P.p32(x), P.p32(x), P.p32(out),
                            C.c_size_t(len(out) if out_points is None else out_points))
            assert (out == 7).all()
            return st
        for K in (0, 1, 3, 6, 12, 24):                           # no power of two, or below 2
            assert level(K, 0, 1, 0, 0) == RR.BAD_OP, K
        for mode in (1, 2):
            for K in (2, 4, 8, 512):                             # the cooperative kernels: 16 <= K <= 256
                assert level(K, 0, 1, 0, mode) == RR.BAD_OP, (mode, K)
        assert level(256, 0, 1, 0, 2) == RR.BAD_OP               # two lanes per point: K <= 128
        assert level(16, 0, 0, 0, 1) == RR.BAD_OP                # nothing to do
        assert level(16, 0, 1, 0, 3) == RR.BAD_OP and level(16, 2, 1, 0, 1) == RR.BAD_OP
        assert level(16, 0, 1 << 18, 0, 1, 1 << 22) == RR.BAD_OP   # more than 2^21 input points
        assert level(16, 0, (1 << 13) + 1, 15, 1, 1 << 22) == RR.BAD_OP    # ... older arrays counted
        assert level(16, 1, 3, 2, 1, 3 * 8) == RR.BAD_OP         # the arrays and the preset behind them need 3 * 9 points
        if g.g2:
            assert level(16, 0, 1, 0, 2) == RR.BAD_OP and level(256, 0, 1, 0, 1) == RR.BAD_OP and level(256, 0, 1, 0, 0) == RR.BAD_OP
            assert RR.probe_plan(host(), g, 5000, 13, tbl=1) == RR.BAD_OP      # G2 is table-free
        assert RR.probe_plan(host(), g, 5000, 1) == RR.BAD_OP and RR.probe_plan(host(), g, 5000, 25) == RR.BAD_OP
        assert RR.probe_plan(host(), g, 5000, 13, glv=1) == RR.BAD_OP and RR.probe_plan(host(), g, 5000, 13, subs=5) == RR.BAD_OP
        assert RR.probe_plan(host(), g, 0, 13) == RR.BAD_OP
    assert host().raw("pc_probe_reduce_level", 5, u(16), u(0), u(1), u(0), C.c_int(1), P.p32(x), P.p32(x), P.p32(x), C.c_size_t(64)) == RR.BAD_OP
    # a plan the level kernels cannot run is refused as a whole: G2 with cooperative groups of 256
    g = RR.Group("bls12_381_g2")
    kn = RR.knob_array({"K1": 256})
    st = host().raw("pc_probe_reduce_all", g.id, C.c_size_t(5000), u(9), u(0), u(0), u(0), kn.ctypes.data_as(C.POINTER(C.c_uint64)), P.p32(x), P.p32(x),
                    P.p32(x))
    assert st == RR.BAD_OP and RR.plan(g, 5000, 9, K1=256).levels[0][0] == 256
