"""The MSM's bucket sort on the device, directly: HipBackend::sort_entries through the test-only probe (tests/hip/probe_sort.hip) against
the reference of its contract (tests/harness/sortref.py), in every regime its geometry has -- the LDS sort with the small and the large
coarse histogram, the atomic sort the library falls back to, every window width, the four modes -- and whole MSMs through the C ABI at
the edges between the regimes.

Every sort's output passes the three exact checks of sortref.check_sort: CSR (offsets are the prefix sums of the reference's bucket
sizes), content (every bucket's entries as a sorted multiset) and reconstruction (from the output alone: every digit once, the digits
sum to the scalar, or to halves that recombine to it).  The probe reports which sort ran; each test asserts the path it is about."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from harness import probe as P
from harness import sortref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = list(S.CURVES)
LDS, ATOMIC = 0, 1
BAD_OP = -2                                             # PROBE_BAD_OP (tests/hip/probe_runner.hpp)
GEOM_FIELDS = "cb fine_bits top_fine_bits NC nblocks S lds lanes fallback W Wd nb_win NB ncw top_w".split()


def u32(v):
    return C.c_uint32(int(v))


@functools.lru_cache(None)
def dev():
    import poly_commit_amd as pc
    pc.load_library()          # brings torch's bundled HIP runtime up first (see load_library), whichever test file runs first
    return P.device_probe()


def geom_of(g):
    """what the production make_sort_geom / sort_needs_atomic / sort_pass_threads give for the call"""
    out = np.zeros(16, dtype=np.uint32)
    dev().call("pc_probe_sort_geom", S.CURVES[g.curve], C.c_size_t(g.n), u32(g.c), u32(g.W), u32(g.Wd), u32(g.tbl_stride),
                          u32(g.m_sub), u32(g.glv), P.p32(out))
    d = dict(zip(GEOM_FIELDS, (int(v) for v in out)))
    assert (d["W"], d["Wd"], d["nb_win"], d["NB"]) == (g.W, g.Wd, g.nb_win, g.NB)
    return d


def mont(curve, canon):
    return np.ascontiguousarray(O.f_to_mont(curve, 1, np.ascontiguousarray(canon).view(np.uint64))).view(np.uint32).reshape(canon.shape)


def run_sort(g, canon, from_mont=0, mode=0, use_tab=0):
    sc = mont(g.curve, canon) if from_mont else np.ascontiguousarray(canon)
    offsets, entries, path = np.zeros(g.NB + 1, dtype=np.uint32), np.zeros(g.n * g.Wd, dtype=np.uint32), np.full(1, 9, dtype=np.uint32)
    dev().call("pc_probe_sort", S.CURVES[g.curve], C.c_size_t(g.n), u32(g.c), u32(g.W), u32(g.Wd), u32(g.tbl_stride), u32(g.m_sub),
                          u32(g.glv), u32(from_mont), u32(g.base_off), mode, use_tab, P.p32(sc), P.p32(offsets), P.p32(entries), P.p32(path))
    return offsets, entries, int(path[0])


def sort_and_check(g, canon, want_path, from_mont=0, mode=0, use_tab=0):
    offsets, entries, path = run_sort(g, canon, from_mont, mode, use_tab)
    assert path == want_path, "%r: path %d, want %d" % (g, path, want_path)
    return S.check_sort(g, canon, offsets, entries)


@functools.lru_cache(None)
def uniform(curve, n, seed=1):
    a = S.uniform(curve, n, seed)
    a.setflags(write=False)
    return a


def table(curve, n, c, glv=0, base_off=0, m_sub=0):
    return S.Geom(curve, n, c, tbl_stride=(m_sub or n) + base_off, m_sub=m_sub, glv=glv, base_off=base_off)


# ---- the boundaries between the regimes, pinned to the production functions -------------------------------------------------------------

def test_geometry_table():
    """BN254 (254-bit scalars).  Table-free c = 19: 14 windows x 2^10 coarse bins = 14336 counters, 56 KiB, 1024 lanes, LDS sort;
    c = 20 (the automatic width of 2^24 pairs): 13 x 2^11 = 26624 bins, atomic.  Many-MSM rows at c = 8 (one bin per row): 8192 is the
    last shape with a 32 KiB histogram and 256 lanes, 8193 the first with 1024; 16384 is exactly 64 KiB and the last LDS shape, 16385
    falls back.  1024 rows of 4096 at the table's c = 13: 16 bins per row, 16384; 1025 rows: 16400, atomic.  Table c = 23: 2^14 bins of
    2^8 buckets, 64 KiB; its GLV form 2 x 2^13 bins of 2^9.  Hyrax's 2048 x 4096: 32768 bins, atomic.  No launch asks for more than
    64 KiB: every shape above it falls back."""
    def q(g):
        d = geom_of(g)
        return d["NC"], d["lds"], d["lanes"], d["fallback"]
    assert q(S.Geom("bn254", 5000, 19)) == (14336, 56 << 10, 1024, 0)
    assert q(S.Geom("bn254", 5000, 18)) == (15 * 512, 30 << 10, 256, 0)
    assert q(S.Geom("bn254", 5000, 20)) == (26624, 104 << 10, 1024, 1)
    d = geom_of(S.Geom("bn254", 1 << 24, 20))
    assert (d["W"], d["cb"], d["NC"], d["fallback"], d["nblocks"]) == (13, 11, 26624, 1, 512)
    for rows, want in ((8192, (8192, 32 << 10, 256, 0)), (8193, (8193, 8193 * 4, 1024, 0)), (16384, (16384, 64 << 10, 1024, 0)),
                       (16385, (16385, 16385 * 4, 1024, 1)), (20000, (20000, 80000, 1024, 1))):
        assert q(table("bn254", rows * 4, 8, m_sub=4)) == want
        assert q(table("bn254", rows * 4, 9, m_sub=4)) == want
    assert q(table("bn254", 1024 * 4096, 13, m_sub=4096)) == (16384, 64 << 10, 1024, 0)
    assert q(table("bn254", 1025 * 4096, 13, m_sub=4096)) == (16400, 65600, 1024, 1)
    assert q(table("bn254", 2048 * 4096, 13, m_sub=4096))[::3] == (32768, 1)
    d = geom_of(table("bn254", 5000, 23))
    assert (d["cb"], d["fine_bits"], d["NC"], d["lds"], d["lanes"], d["fallback"]) == (14, 8, 16384, 64 << 10, 1024, 0)
    d = geom_of(table("bn254", 5000, 23, glv=1))
    assert (d["cb"], d["fine_bits"], d["NC"], d["lds"], d["fallback"]) == (13, 9, 16384, 64 << 10, 0)
    # the top window's own fine width, and a top window without scalar bits where c divides the width
    d = geom_of(S.Geom("bls12_381", 5000, 17))
    assert (d["W"], d["top_w"], d["top_fine_bits"], d["fine_bits"]) == (16, 15, 0, 8)
    d = geom_of(S.Geom("bls12_377", 5000, 11))
    assert (d["W"], d["top_w"], d["top_fine_bits"]) == (24, 23, 0)
    d = geom_of(S.Geom("bls12_381", 5000, 16))          # 15 scalar bits in the top window: the common fine width
    assert (d["top_fine_bits"], d["fine_bits"], d["cb"]) == (8, 8, 7)
    d = geom_of(S.Geom("bls12_381", 5000, 13))          # 8 bits: 2^4 coarse bins of 2^4 buckets
    assert (d["top_fine_bits"], d["fine_bits"], d["cb"]) == (4, 8, 4)
    # nothing outside the preconditions is accepted: a width out of range, another W or Wd than the builder's, a base index of 2^31
    pr, out = dev(), np.zeros(16, dtype=np.uint32)
    for n, c, W, Wd, stride in ((5000, 1, 255, 255, 0), (5000, 25, 11, 11, 0), (5000, 19, 13, 14, 0), (5000, 19, 14, 13, 0), (5000, 23, 1, 12, 1 << 28)):
        assert pr.raw("pc_probe_sort_geom", 1, C.c_size_t(n), u32(c), u32(W), u32(Wd), u32(stride), u32(0), u32(0), P.p32(out)) == BAD_OP


# ---- the direct sweep --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", range(3, 20))
@pytest.mark.parametrize("curve", CURVES)
def test_sweep_table_free(curve, c):
    """n = 5000 uniform scalars at every width up to 19, the last the LDS sort takes table-free; canonical and Montgomery input and a
    base offset by turns"""
    g = S.Geom(curve, 5000, c, base_off=(c % 3) * 1234)
    assert sort_and_check(g, uniform(curve, 5000), LDS, from_mont=c & 1) > 5000


@pytest.mark.parametrize("c", [8, 13, 16, 20, 23])
@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("curve", CURVES)
def test_sweep_window_table(curve, glv, c):
    """one shared bucket set (W = 1) and the GLV table's two (W = 2); c = 23 is the 64 KiB coarse histogram"""
    g = table(curve, 5000, c, glv=glv, base_off=(c % 2) * 77)
    assert c != 23 or geom_of(g)["lds"] == 64 << 10
    assert sort_and_check(g, uniform(curve, 5000), LDS, from_mont=(c >> 1) & 1) > 5000


MANY = [(37, 200, 9), (8192, 4, 8), (8193, 4, 8), (16384, 4, 8)]


@pytest.mark.parametrize("rows,m,c", MANY)
@pytest.mark.parametrize("curve", CURVES)
def test_sweep_many(curve, rows, m, c):
    """many-MSM mode up to the last row count of the LDS sort, the scalar vectors as one array and through a table of their
    addresses; every 16th row is zero and row 1 holds r - 1 throughout"""
    g = table(curve, rows * m, c, m_sub=m, base_off=3)
    canon = uniform(curve, rows * m, 2).copy().reshape(rows, m, S.FR_WORDS)
    canon[::16] = 0
    canon[1] = S.to_limbs([S.modulus(curve) - 1])[0]
    canon = canon.reshape(rows * m, S.FR_WORDS)
    sort_and_check(g, canon, LDS, from_mont=1)
    sort_and_check(g, canon, LDS, use_tab=1)
    if rows == 37:
        sort_and_check(table(curve, rows * m, c, m_sub=m, glv=1), canon, LDS, use_tab=1)


def mode_geom(mode, curve, n):
    """one width per mode: table-free c = 13, table c = 16, GLV table c = 13, 3 rows at c = 9; above 2^20 pairs the widths with the
    fewest digits the LDS sort takes: 19, 23, 23 and 16"""
    if mode == "plain":
        return S.Geom(curve, n, 19 if n > 1 << 20 else 13)
    if mode == "many":
        return table(curve, 3 * n, 16 if n > 1 << 18 else 9, m_sub=n)
    return table(curve, n, 23 if n > 1 << 20 else 16 if mode == "table" else 13, glv=int(mode == "glv"))


@pytest.mark.parametrize("n", [1, 31, 2047, 2048, 2049, 70001])
@pytest.mark.parametrize("mode", ["plain", "table", "glv", "many"])
@pytest.mark.parametrize("curve", CURVES)
def test_sort_block_edges(curve, mode, n):
    """one pair, fewer pairs than lanes, one sort block and one pair either side of it, and 35 blocks of 2001 with 1024 lanes"""
    g = mode_geom(mode, curve, n)
    d = geom_of(g)
    assert d["nblocks"] == min(512, (g.n + 2047) // 2048) and d["lanes"] == (1024 if g.n >= 65536 else 256)
    sort_and_check(g, uniform(curve, g.n, 3), LDS, from_mont=n & 1)


@pytest.mark.parametrize("mode", ["plain", "table", "glv", "many"])
@pytest.mark.parametrize("curve", CURVES)
def test_more_pairs_than_the_block_grid_holds(curve, mode):
    """n above 512 * 2048: the 512 blocks take more than 2048 scalars each (the checks walk 13 M to 17 M entries: the slowest cases here)"""
    n = 512 * 2048 + 4097 if mode != "many" else (512 * 2048) // 3 + 1367
    g = mode_geom(mode, curve, n)
    d = geom_of(g)
    assert d["nblocks"] == 512 and d["S"] > 2048 and not d["fallback"]
    pool = uniform(curve, 1 << 14, 4)                  # (drawn from a pool: the GLV reference splits each distinct scalar once)
    canon = pool[np.random.RandomState(5).randint(0, len(pool), size=g.n)]
    sort_and_check(g, canon, LDS)


# ---- scalar sets -------------------------------------------------------------------------------------------------------------------

SET_SHAPES = [("plain", 5), ("plain", 11), ("plain", 17), ("plain", 19), ("table", 13), ("table", 23), ("glv", 16), ("glv", 23), ("many", 9)]
RUNS = (511, 512, 513, 2047, 2048, 2049, 4097)


def shaped(mode, curve, n, c):
    if mode == "plain":
        return S.Geom(curve, n, c)
    if mode == "many":                                  # the set in rows 0 and 2, zeros between them
        return table(curve, 3 * n, c, m_sub=n)
    return table(curve, n, c, glv=int(mode == "glv"))


def as_call(mode, canon):
    return np.concatenate([canon, np.zeros_like(canon), canon]) if mode == "many" else canon


@pytest.mark.parametrize("mode,c", SET_SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_scalar_sets(curve, mode, c):
    """all zero (every offset 0); all r - 1; one scalar n times -- n entries in one bucket per window, n on both sides of the fine
    pass's 512 lanes and four-in-flight loop (2048 records) -- for a random scalar, for the scalar whose every digit is 2^(c-1) (last
    bucket, no carry) and for the one whose every digit is 2^(c-1) + 1 (a carry through every window into the top one); the edge
    scalars (0, 1, r - 1, 2^k, 2^k - 1 for every k, ...); scalars whose top window is empty.  The widths include those that divide
    the scalar's bits (5 and 17: 255; 11 and 23: 253), where the top window holds a carry or nothing."""
    r, bits = S.modulus(curve), S.FR_BITS[curve]
    half = 1 << (c - 1)

    def run(vals_or_limbs, from_mont=0):
        canon = vals_or_limbs if isinstance(vals_or_limbs, np.ndarray) else S.to_limbs(vals_or_limbs)
        g = shaped(mode, curve, len(canon), c)
        offsets, entries, path = run_sort(g, as_call(mode, canon), from_mont)
        assert path == LDS
        return S.check_sort(g, as_call(mode, canon), offsets, entries), offsets
    M, offsets = run([0] * 2049)
    assert M == 0 and not offsets.any()
    run([r - 1] * 2049, from_mont=1)
    rnd = S.to_ints(uniform(curve, 1, 6))[0]
    for n in RUNS:
        run([rnd] * n, from_mont=n & 1)
    for v in (S.pattern(half, c, bits, r), S.pattern(half + 1, c, bits, r)):
        for n in (513, 2049, 4097):
            run([v] * n)
    edge = S.edge_scalars(curve, c, mode == "glv")
    run(edge)
    run(edge, from_mont=1)
    run(S.uniform(curve, 3000, 7, bits=c * ((S.HALF_BITS if mode == "glv" else bits) // c) - 1))


# ---- the atomic sort ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [20, 22, 24])
@pytest.mark.parametrize("curve", CURVES)
def test_fallback_table_free(curve, c):
    """table-free widths above 19: more coarse bins than the 64 KiB histogram holds (c = 20, 22) or more fine buckets than the fine
    pass's (c = 24); uniform and edge scalars"""
    assert geom_of(S.Geom(curve, 5000, c))["fallback"] == 1
    sort_and_check(S.Geom(curve, 5000, c, base_off=9), uniform(curve, 5000), ATOMIC, from_mont=1)
    edge = S.to_limbs(S.edge_scalars(curve, c))
    sort_and_check(S.Geom(curve, len(edge), c), edge, ATOMIC)


@pytest.mark.parametrize("rows", [16385, 20000])
@pytest.mark.parametrize("curve", CURVES)
def test_fallback_many(curve, rows):
    """more bucket sets than coarse counters: the first such row count and 20000, plain array and address table"""
    g = table(curve, rows * 4, 8, m_sub=4, base_off=3)
    assert geom_of(g)["fallback"] == 1
    canon = uniform(curve, rows * 4, 2).copy()
    canon[::64] = 0
    sort_and_check(g, canon, ATOMIC, from_mont=1)
    sort_and_check(g, canon, ATOMIC, use_tab=1)


def buckets(offsets, entries):
    M = int(offsets[-1])
    key = np.searchsorted(offsets, np.arange(M, dtype=np.int64), side="right") - 1
    return np.sort((key.astype(np.uint64) << np.uint64(32)) | entries[:M].astype(np.uint64))


@pytest.mark.parametrize("curve", CURVES)
def test_forced_atomic_agrees_with_the_lds_sort(curve):
    """at LDS-sort shapes of every mode the probe's mode 1 runs the atomic sort: the same offsets and, bucket for bucket, the same
    entries; and the atomic sort passes the checks on its own"""
    for g in (S.Geom(curve, 5000, 13, base_off=5), S.Geom(curve, 5000, 19), table(curve, 5000, 16), table(curve, 5000, 23, glv=1),
              table(curve, 37 * 200, 9, m_sub=200), table(curve, 37 * 200, 9, m_sub=200, glv=1), table(curve, 16384 * 4, 8, m_sub=4)):
        canon = uniform(curve, g.n, 8)
        o0, e0, p0 = run_sort(g, canon, mode=0)
        o1, e1, p1 = run_sort(g, canon, mode=1)
        assert (p0, p1) == (LDS, ATOMIC), g
        assert np.array_equal(o0, o1) and np.array_equal(buckets(o0, e0), buckets(o1, e1)), g
        S.check_sort(g, canon, o1, e1)


# ---- whole MSMs at the edges of the regimes ----------------------------------------------------------------------------------------

POOL, M_MANY = 64, 4


@functools.lru_cache(None)
def many_pool(curve):
    """64 scalar vectors of 4 -- a zero row, an r - 1 row, an equal-scalar row among them -- and the oracle's point of each"""
    bases = O.gen_bases(curve, M_MANY)
    r = S.modulus(curve)
    vecs = S.uniform(curve, POOL * M_MANY, 11).reshape(POOL, M_MANY, S.FR_WORDS)
    vecs[0] = 0
    vecs[1] = S.to_limbs([r - 1])[0]
    vecs[2] = vecs[2, 0]
    vecs = np.ascontiguousarray(vecs).view(np.uint64).reshape(POOL, M_MANY, 4)
    want = np.stack([O.msm_naive(curve, bases, np.ascontiguousarray(v)) for v in vecs])
    assert want[1:].any(axis=1).all() and not want[0].any()
    return bases, vecs, want


def sort_regime(curve, shape, n, m_sub=0):
    """the regime of the call the library just made, from its reported shape"""
    c, tab = shape["window_bits"], shape["window_table"]
    glv = int(tab and shape["buckets"] == (2 if not m_sub else 2 * n // m_sub) << (c - 1))
    g = table(curve, n, c, glv=glv, m_sub=m_sub) if tab else S.Geom(curve, n, c)
    assert shape["buckets"] == g.NB and shape["digits_per_scalar"] == g.Wd
    return geom_of(g)


@pytest.mark.parametrize("n_msms", [8192, 8193, 16384, 16385, 20000])
def test_msm_many_across_the_row_limits(ctx, n_msms):
    """pc_hip_msm_many on BN254, m = 4: the last shape of the 32 KiB histogram, the first of the 1024-lane pass, the last LDS shape,
    the first atomic one and 20000 rows.  Rows are drawn from the pool; every row and every infinity flag is compared; host scalars
    (canonical) and device scalars (Montgomery)."""
    import torch
    curve = "bn254"
    bases, vecs, want = many_pool(curve)
    idx = np.random.RandomState(n_msms).randint(0, POOL, size=n_msms)
    idx[:3] = (0, 1, 2)
    rows, exp = np.ascontiguousarray(vecs[idx]), want[idx]
    srs = ctx.upload_srs(curve, bases)
    try:
        got, inf = srs.msm_many(rows)
        d = sort_regime(curve, ctx.last_msm_shape(), n_msms * M_MANY, M_MANY)
        assert d["fallback"] == int(n_msms > 16384) and d["lanes"] == (1024 if n_msms > 8192 else 256) and d["NC"] == n_msms * d["ncw"]
        assert (got == exp).all(), [k for k in range(n_msms) if not (got[k] == exp[k]).all()][:8]
        assert np.array_equal(inf, ~exp.any(axis=1))
        dev = torch.from_numpy(O.f_to_mont(curve, 1, rows).view(np.int64)).cuda()
        got, inf = srs.msm_many(dev.data_ptr(), m=M_MANY, n_msms=n_msms, montgomery=True)
        assert (got == exp).all() and np.array_equal(inf, ~exp.any(axis=1))
    finally:
        srs.free()


def test_te_msm_many_past_the_row_limit(ctx):
    """pc_hip_te_msm_many on ed_on_bls12_381, 16385 x 4: the atomic sort under the twisted Edwards many-MSM pass, against teref"""
    import torch
    from harness import teref as E
    curve, n_msms = "ed_on_bls12_381", 16385
    pts = E.fixed_base(E.GEN).mul_many([(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % E.R for i in range(M_MANY)])
    rnd = np.random.RandomState(12)
    pool = [[int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(M_MANY)] for _ in range(POOL)]
    pool[0], pool[1], pool[2] = [0] * M_MANY, [E.R - 1] * M_MANY, [pool[2][0]] * M_MANY
    want = [E.msm(pts, r) for r in pool]
    assert want[0] == E.IDENT and all(w != E.IDENT for w in want[1:])
    idx = rnd.randint(0, POOL, size=n_msms)
    idx[:3] = (0, 1, 2)

    def same_rows(got, ident):
        """every row: the rows of one pool vector are the same bytes, and those bytes are the vector's point"""
        assert np.array_equal(ident, idx == 0)
        for j in range(POOL):
            rows = got[idx == j]
            assert len(rows) and (rows == rows[0]).all(), j
            assert E.point_from_bytes(rows[0].tobytes()) == want[j], j
        assert got[0].tobytes() == E.IDENT_BYTES
    key = ctx.upload_te_srs(curve, E.points_array(pts))
    try:
        for montg in (False, True):
            arr = E.scalars_array([k for r in pool for k in r], montg).reshape(POOL, M_MANY, 32)[idx]
            got, ident = key.msm_many(np.ascontiguousarray(arr), montgomery=montg)
            same_rows(got, ident)
        dev = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        same_rows(*key.msm_many(dev, m=M_MANY, n_msms=n_msms, montgomery=True))
        shape = ctx.last_msm_shape()
        assert shape["window_table"] and shape["buckets"] == n_msms << (shape["window_bits"] - 1)
    finally:
        key.free()


@functools.lru_cache(None)
def single_case(curve):
    bases, sc = O.gen_bases(curve, 5000), O.gen_scalars(curve, 0x50F7, 5000)
    return bases, sc, O.msm_pippenger(curve, bases, sc)


@pytest.mark.parametrize("c", [14, 15, 17, 19, 20])
@pytest.mark.parametrize("curve", ["bn254", "bls12_377"])
def test_single_msm_at_the_widths_the_tunings_skip(ctx, curve, c):
    """5000 pairs table-free under set_msm_tuning(c): 19 is the 56 KiB coarse pass, 20 the atomic sort (6.8 M buckets)"""
    bases, sc, want = single_case(curve)
    ctx.set_msm_tuning(c, 0)
    try:
        srs = ctx.upload_srs(curve, bases)
        try:
            got, inf = srs.msm(sc)
            shape = ctx.last_msm_shape()
            assert shape["window_bits"] == c and not shape["window_table"]
            d = sort_regime(curve, shape, 5000)
            assert d["fallback"] == int(c == 20) and (c != 19 or d["lds"] == 56 << 10)
            assert (got == want).all() and not inf
            got, inf = srs.msm(O.f_to_mont(curve, 1, sc), montgomery=True)
            assert (got == want).all() and not inf
        finally:
            srs.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("glv", [False, True])
def test_window_table_of_23_bits(ctx, glv):
    """precompute(window_bits = 23) on 5000 BN254 bases: the coarse histogram of exactly 64 KiB, plain and GLV table"""
    curve = "bn254"
    bases, sc, want = single_case(curve)
    srs = ctx.upload_srs(curve, bases)
    try:
        srs.precompute(window_bits=23, min_pairs=1, glv=glv)
        got, inf = srs.msm(sc)
        shape = ctx.last_msm_shape()
        assert shape["window_bits"] == 23 and shape["window_table"] and shape["buckets"] == (2 if glv else 1) << 22
        d = sort_regime(curve, shape, 5000)
        assert (d["lds"], d["lanes"], d["fallback"]) == (64 << 10, 1024, 0)
        assert (got == want).all() and not inf
    finally:
        srs.free()


CHILD_ATOMIC = r'''
import sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import oracle_lib as O
import poly_commit_amd as pc
ctx = pc.Context(0)
for curve in ("bn254", "bls12_381"):
    n = 5000
    bases, sc = O.gen_bases(curve, n), O.gen_scalars(curve, 0xA70, n)
    want = O.msm_pippenger(curve, bases, sc)
    srs = ctx.upload_srs(curve, bases)
    got, inf = srs.msm(sc)
    assert (got == want).all() and not inf, (curve, "plain")
    got, inf = srs.msm(O.f_to_mont(curve, 1, sc), montgomery=True, base_offset=0)
    assert (got == want).all(), (curve, "plain, Montgomery")
    rows = np.ascontiguousarray(sc[:4800].reshape(24, 200, 4))
    wants = np.stack([O.msm_naive(curve, bases[:200], np.ascontiguousarray(r)) for r in rows])
    got, inf = srs.msm_many(rows)
    assert (got == wants).all() and not inf.any(), (curve, "many")
    srs.free()
    for glv in (False, True):
        srs = ctx.upload_srs(curve, bases)
        srs.precompute(min_pairs=1, glv=glv)
        got, inf = srs.msm(sc)
        shape = ctx.last_msm_shape()
        assert shape["window_table"] and shape["buckets"] == (2 if glv else 1) << (shape["window_bits"] - 1), (curve, glv, shape)
        assert (got == want).all() and not inf, (curve, "table", glv)
        srs.free()
ctx.close()
print("atomic ok")
'''


def test_whole_msms_on_the_atomic_sort():
    """PC_HIP_SORT=atomic (read once per backend: a child process): a plain MSM, a many-MSM pass, and an MSM over the window table and
    over the GLV table, each against the oracle"""
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD_ATOMIC], env=dict(os.environ, PC_HIP_SORT="atomic"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "atomic ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
