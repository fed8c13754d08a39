"""G1 MSMs whose sums become the point at infinity INSIDE the pipeline: pc_hip_msm (table-free, over the window table in its plain and
GLV form, host scalars in parts), pc_hip_msm_many and the fast path of pc_hip_msm_batch, on all four curves through the C ABI, bit for
bit against an expectation made of Python integers.

The keys (tests/harness/signedkey.py) hold P beside -P with known logarithms, so every result is (sum_j s_j e_j mod r) G: one scalar
multiplication, all-zero words and the infinity flag where the sum is 0 mod r.  The scalar layouts put P and -P under the SAME digit:
the running sum of a lane passes through infinity and goes on, whole chunks sum to infinity and are written to their partial-sum slot
as such, the joins (the in-workgroup scan of k_accumulate, k_accumulate_edges, the segmented reduction, the two-lane additions of the
bucket reduction) meet P + (-P), infinite operands and -- on the one-base key -- equal operands, and in many-MSM mode bucket sets that
hold nothing but cancelled sums lie beside sets that hold points.  tests/test_signedkey_cpu.py holds the oracle's two MSMs against the
same expectation, tests/test_emu_cpu.py steps the small shapes on the CPU.

Before the cancelling calls every pipeline of a key runs a call with random scalars: it leaves a point in every partial-sum slot, so
an infinity that a later call does not WRITE to its slot shows as a wrong result.  The chunk length of a call is not part of its
reported shape; that set_msm_tuning(0, T) reaches a single MSM and the batch passes (but not pc_hip_msm_many, which sets T = 0) is
read from MsmPlan::part_body, where cfg_.T goes straight into g.T."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from harness import signedkey as SK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = SK.CURVES
SIGNED = ("const", "pairwise", "pairwise_few", "all_but_one")
LANES = 3                                                   # pipelines of a key (PC_MSM_LANES): blocking calls take them in rotation


def _is(got, want, what):
    out, inf = got
    assert (out == want).all(), what
    assert bool(inf) == (not want.any()), what


def _cases(curve, n):
    """[(key, random scalars, its point, {layout: (words, expected point)})] for the signed key with holes, the unsigned key under
    opposite scalars and the one-base key under one scalar; the first entry is the one every tuning runs"""
    out = []
    for key, names, holes in ((SK.signed(curve, n, holes=True), SIGNED, True), (SK.unsigned(curve, n), ("opposite_scalars",), False),
                              (SK.one_base(curve, n), ("const",), False)):
        lay = SK.layouts(curve, n, 0xCA5E + n, 0, holes)
        rnd = SK.rand_scalars(curve, n, 0xCA5F + n)
        sets = {name: (SK.limbs(lay[name]), SK.expected(key, lay[name])) for name in names}
        out.append((key, SK.limbs(rnd), SK.expected(key, rnd), sets))
    signed, unsigned, one = out
    assert all(w.any() == (name == "all_but_one") for name, (_, w) in signed[3].items())
    assert not unsigned[3]["opposite_scalars"][1].any() and one[3]["const"][1].any()
    for key, _, _, sets in out:                             # second opinion: the oracle's bucket method
        for name, (sc, want) in sets.items():
            assert (O.msm_pippenger(curve, key.bases, sc, 8, 1) == want).all(), name
    return out


def _run_key(ctx, curve, case, what, table=None):
    """one upload under the tuning that is set now; random scalars on every pipeline, then every layout of the key"""
    key, rnd, rnd_want, sets = case
    srs = ctx.upload_srs(curve, key.bases)
    try:
        if table is not None:
            srs.precompute(min_pairs=1, glv=table)
        for _ in range(LANES):
            _is(srs.msm(rnd), rnd_want, (what, "random"))
        for name, (sc, want) in sets.items():
            _is(srs.msm(sc), want, (what, name))
            if table is not None:
                assert ctx.last_msm_shape()["window_table"]
    finally:
        srs.free()


@pytest.mark.parametrize("n", [64, 700, 5000])
@pytest.mark.parametrize("curve", CURVES)
def test_single_msm_table_free(ctx, curve, n):
    """signed(n, holes=True) under const, pairwise, pairwise_few (infinity) and all_but_one (a known point) with the automatic chunk and
    chunks of 1, 2, 5 and 8 entries: under an even chunk length most chunks of `const` sum to infinity, under an odd one they alternate
    +-k P and cancel in the joins; at n = 5000 a bucket of `const` spans several workgroups of the accumulation.  The controls at
    T = 0 and 5: opposite scalars on the unsigned key cancel only behind the buckets, one scalar on one base makes the joins double."""
    signed, unsigned, one = _cases(curve, n)
    try:
        for T in (0, 1, 2, 5, 8):
            ctx.set_msm_tuning(0, T)
            _run_key(ctx, curve, signed, (curve, n, T))
            if T in (0, 5):
                _run_key(ctx, curve, unsigned, (curve, n, T, "unsigned"))
                _run_key(ctx, curve, one, (curve, n, T, "one base"))
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("c,T", [(4, 1), (13, 64)])
@pytest.mark.parametrize("curve", CURVES)
def test_single_msm_window_tunings(ctx, curve, c, T):
    """two of test_msm_tunings' settings on `const` and `all_but_one` at n = 5000; the width is read back from the call's shape"""
    n = 5000
    key = SK.signed(curve, n, holes=True)
    lay = SK.layouts(curve, n, 0xCA60, 0, holes=True)
    rnd = SK.rand_scalars(curve, n, 0xCA61)
    ctx.set_msm_tuning(c, T)
    try:
        srs = ctx.upload_srs(curve, key.bases)
        try:
            for _ in range(LANES):
                _is(srs.msm(SK.limbs(rnd)), SK.expected(key, rnd), (curve, c, T, "random"))
            for name in ("const", "all_but_one"):
                _is(srs.msm(SK.limbs(lay[name])), SK.expected(key, lay[name]), (curve, c, T, name))
                shape = ctx.last_msm_shape()
                assert shape["window_bits"] == c and not shape["window_table"]
        finally:
            srs.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("glv", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_single_msm_over_the_window_table(ctx, curve, glv):
    """n = 5000 over the window table, plain and GLV form (both members of a pair split alike, so both bucket sets cancel), chunks of
    0 (automatic), 2 and 5 entries, every layout on its key"""
    cases = _cases(curve, 5000)
    try:
        for T in (0, 2, 5):
            ctx.set_msm_tuning(0, T)
            for case in cases:
                _run_key(ctx, curve, case, (curve, glv, T), table=glv)
    finally:
        ctx.set_msm_tuning(0, 0)


# ---- pc_hip_msm_many --------------------------------------------------------------------------------------------------------------------

def _many(srs, curve, key, rows, off, what, montgomery=False, device=False):
    """rows of integers through pc_hip_msm_many against the integer expectation; returns the flags"""
    want = np.stack([SK.expected(key, r, off) for r in rows])
    mat = np.ascontiguousarray(np.stack([SK.mont(curve, r) if montgomery else SK.limbs(r) for r in rows]))
    if device:
        import torch
        dev = torch.from_numpy(mat.view(np.int64)).cuda()
        got, inf = srs.msm_many(dev.data_ptr(), m=mat.shape[1], n_msms=len(rows), base_offset=off, montgomery=montgomery)
    else:
        got, inf = srs.msm_many(mat, base_offset=off, montgomery=montgomery)
    assert (got == want).all(), (what, [k for k in range(len(rows)) if not (got[k] == want[k]).all()])
    assert list(inf) == [not w.any() for w in want], what
    return list(inf)


def _random_rows(curve, m, B, seed):
    return [SK.rand_scalars(curve, m, seed + k) for k in range(B)]


@pytest.mark.parametrize("off", [0, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_msm_many_rows_that_cancel_beside_rows_that_do_not(ctx, curve, off):
    """m = 200, B = 6 over signed(m + 7, holes=True): [random, const, copy of row 0, all_but_one, pairwise_few, zeros] -- bucket sets
    sub * 2^(c-1) + bucket that hold nothing but cancelled sums between sets that hold points, in one workgroup; the same rows with
    the cancelling ones first and last; five `const` rows of different scalars: exactly zero words.  Canonical and Montgomery scalars,
    host and device memory."""
    m = 200
    key = SK.signed(curve, m + 7, holes=True)
    lay = SK.layouts(curve, m, 0xCA62, off, holes=True)
    rnd = SK.rand_scalars(curve, m, 0xCA63)
    rows = [rnd, lay["const"], list(rnd), lay["all_but_one"], lay["pairwise_few"], [0] * m]
    srs = ctx.upload_srs(curve, key.bases)
    try:
        _many(srs, curve, key, _random_rows(curve, m, 6, 0xCA64), off, "random")          # a point in every slot of the pass's pipeline
        assert _many(srs, curve, key, rows, off, "rows") == [False, True, False, False, True, True]
        assert _many(srs, curve, key, rows, off, "rows, Montgomery", montgomery=True) == [False, True, False, False, True, True]
        perm = [1, 0, 3, 2, 5, 4]
        _many(srs, curve, key, _random_rows(curve, m, 6, 0xCA65), off, "random")
        assert _many(srs, curve, key, [rows[k] for k in perm], off, "permuted", device=True) == [True, False, False, False, True, True]
        consts = [SK.const(curve, m, 0xCA66 + k, off, holes=True) for k in range(5)]
        assert len({max(r) for r in consts}) == 5
        _many(srs, curve, key, _random_rows(curve, m, 5, 0xCA67), off, "random")
        assert _many(srs, curve, key, consts, off, "five const rows") == [True] * 5
    finally:
        srs.free()


@pytest.mark.parametrize("off", [0, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_msm_many_one_bucket_spans_workgroups(ctx, curve, off):
    """m = 5000, B = 3: [const, const with one scalar changed, random].  One bucket per window holds (nearly) all 5000 entries of rows 0
    and 1.  The pass builds its own table with msm_choose_table_c(5000, bits, 0) = 13 (20 digits per scalar for 253 .. 255 bits:
    5000 * 20 + 3 * 2^12 is the minimum of its cost), so 3 * 5000 * 20 = 300 000 entries.  pc_hip_msm_many sets cfg.T = 0: the chunk
    is ceil(300 000 / tbl_target_lanes = 2^17) = 3, raised to the plan's minimum min_T_ = 16 (8 only for plans of at most 2^17
    entries).  A run of 5000 entries is 313 chunks of 16: more than one whole workgroup of the accumulation, so k_accumulate_edges and
    the segmented reduction see chains of infinite (row 0) and of mostly infinite (row 1) partial sums.  The shape is asserted so that
    a change of planning cannot quietly make this another test."""
    m = 5000
    key = SK.signed(curve, m + 7, holes=True)
    rows = [SK.const(curve, m, 0xCA68, off, holes=True), SK.all_but_one_on_const(curve, m, 0xCA68, off, holes=True), SK.rand_scalars(curve, m, 0xCA69)]
    assert sum(1 for a, b in zip(rows[0], rows[1]) if a != b) == 1
    srs = ctx.upload_srs(curve, key.bases)
    try:
        _many(srs, curve, key, _random_rows(curve, m, 3, 0xCA6A), off, "random")
        assert _many(srs, curve, key, rows, off, "rows") == [True, False, False]
        assert ctx.last_msm_shape() == {"window_bits": 13, "digits_per_scalar": 20, "buckets": 3 << 12, "window_table": True}
        assert _many(srs, curve, key, rows[::-1], off, "reversed", montgomery=True, device=True) == [False, False, True]
    finally:
        srs.free()


@pytest.mark.parametrize("curve", CURVES)
def test_msm_many_equal_partial_sums_meet_in_the_joins(ctx, curve):
    """one_base(4096), B = 3, one scalar per row (1, 3, random): the many-mode twin of test_msm_equal_partial_sums_meet_in_the_joins --
    every chunk of a row's bucket sums to the same point, the joins take their doubling branch"""
    m = 4096
    key = SK.one_base(curve, m + 7)
    rows = [[1] * m, [3] * m, SK.rand_scalars(curve, 1, 0xCA6B) * m]
    srs = ctx.upload_srs(curve, key.bases)
    try:
        for off in (0, 7):
            assert _many(srs, curve, key, rows, off, off) == [False] * 3
    finally:
        srs.free()


# ---- pc_hip_msm_batch: many-MSM mode over the key's own table, separate scalar buffers ------------------------------------------------

BATCH_M, BATCH_OFF, BATCH_K = 1 << 14, 5, 11
_batch_sets = {}


def _batch_polys(curve):
    """(key, 11 Montgomery polynomials, their expected points): random, zeros, const, a copy of polynomial 0, all_but_one, pairwise,
    pairwise_few and four more random ones -- made once per curve"""
    if curve not in _batch_sets:
        m, off = BATCH_M, BATCH_OFF
        key = SK.signed(curve, m + off, holes=True)
        lay = SK.layouts(curve, m, 0xCA70, off, holes=True)
        rnd = [SK.rand_scalars(curve, m, 0xCA71 + k) for k in range(5)]
        polys = [rnd[0], [0] * m, lay["const"], list(rnd[0]), lay["all_but_one"], lay["pairwise"], lay["pairwise_few"]] + rnd[1:]
        assert len(polys) == BATCH_K
        want = np.stack([SK.expected(key, p, off) for p in polys])
        assert [not w.any() for w in want] == [False, True, True, False, False, True, True] + [False] * 4
        _batch_sets[curve] = (key, [SK.mont(curve, p) for p in polys], want)
    return _batch_sets[curve]


def _batch(ctx, srs, arrs, lens, off, host):
    """pc_hip_msm_batch with its flags (the binding's msm_batch returns the points only)"""
    from poly_commit_amd import _ffi
    k = len(arrs)
    keep = None
    if host:
        addr = [a.ctypes.data for a in arrs]
    else:
        import torch
        keep = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrs]
        addr = [t.data_ptr() for t in keep]
    out = np.zeros((k, 2 * O.fq_limbs(srs.curve)), dtype=np.uint64)
    infs = (C.c_int * k)()
    ctx.check(ctx.lib.pc_hip_msm_batch(ctx.h, srs.h, (C.c_size_t * k)(*[off] * k), (C.c_void_p * k)(*addr), (C.c_size_t * k)(*lens), k,
                                       _ffi.PC_SCALARS_MONTGOMERY, _ffi.PC_MEM_HOST if host else _ffi.PC_MEM_DEVICE, C.c_void_p(out.ctypes.data), infs))
    del keep
    return out, np.array(list(infs), dtype=bool)


def _batch_under_tunings(ctx, curve, tunings, glv):
    key, polys, want = _batch_polys(curve)
    m, off, k = BATCH_M, BATCH_OFF, BATCH_K
    flags = [not w.any() for w in want]
    dirty = [SK.mont(curve, SK.rand_scalars(curve, m, 0xCA80 + j)) for j in range(8)]
    try:
        for T in tunings:
            ctx.set_msm_tuning(0, T)
            srs = ctx.upload_srs(curve, key.bases)
            try:
                srs.precompute(min_pairs=1, glv=glv)
                # the passes are 8 + 3 on the two pipelines of the batch: two random passes of 8 first, a point in every slot of both
                _batch(ctx, srs, dirty + dirty, [m] * 16, off, host=False)
                for host in (False, True):
                    got, inf = _batch(ctx, srs, polys, [m] * k, off, host)
                    assert (got == want).all(), (curve, T, glv, host, [j for j in range(k) if not (got[j] == want[j]).all()])
                    assert list(inf) == flags, (curve, T, glv, host)
                # the same batch with one more polynomial of another length: unequal lengths, every polynomial on the single-MSM pipelines
                got, inf = _batch(ctx, srs, polys + [np.ascontiguousarray(polys[0][:m - 1])], [m] * k + [m - 1], off, host=False)
                assert (got[:k] == want).all() and list(inf[:k]) == flags, (curve, T, glv, "per polynomial")
            finally:
                srs.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("curve", CURVES)
def test_msm_batch_fast_path_under_chunk_tunings(ctx, curve):
    """m = 2^14 (the shortest length that takes the fast path) over signed(2^14 + 5, holes=True) from offset 5 with the window table,
    11 polynomials = passes of 8 + 3 (the second pass leaves five bucket sets empty).  The plan of a pass is made from the key's own
    configuration, so set_msm_tuning(0, T) before the upload gives many-mode chunks of 1, 2 and 5 entries (pc_hip_msm_many cannot:
    it sets T = 0).  Device buffers and host buffers; the per-polynomial path gives the same points."""
    _batch_under_tunings(ctx, curve, (0, 1, 2, 5) if curve in ("bls12_381", "bls12_377") else (0, 5), glv=False)


@pytest.mark.parametrize("curve", ["bls12_377", "bn254"])
def test_msm_batch_fast_path_over_the_glv_table(ctx, curve):
    """the same over the GLV form of the table (two bucket sets per polynomial, phi on the second set's sum), one curve of twelve and
    one of eight limbs"""
    _batch_under_tunings(ctx, curve, (0, 5), glv=True)


CHILD_HEAD = r'''
import sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import ctypes as C
import numpy as np
from harness import signedkey as SK
import poly_commit_amd as pc
from poly_commit_amd import _ffi
ctx = pc.Context(0)
'''

CHILD_BATCH_G = CHILD_HEAD + r'''
m, off, k = 1 << 14, 5, 5
for curve in SK.CURVES:
    key = SK.signed(curve, m + off, holes=True)
    lay = SK.layouts(curve, m, 0xCA90, off, holes=True)
    rnd = SK.rand_scalars(curve, m, 0xCA91)
    polys = [rnd, lay["const"], lay["all_but_one"], lay["pairwise"], lay["pairwise_few"]]
    want = np.stack([SK.expected(key, p, off) for p in polys])
    arrs = [SK.mont(curve, p) for p in polys]
    srs = ctx.upload_srs(curve, key.bases)
    srs.precompute(min_pairs=1)
    out = np.zeros_like(want)
    infs = (C.c_int * k)()
    for rep in range(2):
        ctx.check(ctx.lib.pc_hip_msm_batch(ctx.h, srs.h, (C.c_size_t * k)(*[off] * k), (C.c_void_p * k)(*[a.ctypes.data for a in arrs]), (C.c_size_t * k)(*[m] * k), k,
                                           _ffi.PC_SCALARS_MONTGOMERY, _ffi.PC_MEM_HOST, C.c_void_p(out.ctypes.data), infs))
        assert (out == want).all(), (curve, rep, [j for j in range(k) if not (out[j] == want[j]).all()])
        assert list(infs) == [0, 1, 0, 1, 1], (curve, list(infs))
    srs.free()
ctx.close()
print("batch-g ok")
'''


@pytest.mark.parametrize("G", ["2", "3"])
def test_msm_batch_remainder_pass_of_one_polynomial(G):
    """PC_HIP_BATCH_G = 2, 3 (read once per process: a child) and five polynomials: passes of 2 + 2 + 1, resp. 3 + 2 -- the remainder
    pass holds fewer polynomials than its plan has bucket sets, a single one for G = 2; twice, so that both pipelines run both kinds"""
    env = dict(os.environ, PC_HIP_BATCH_G=G)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD_BATCH_G], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "batch-g ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


CHILD_PARTS = CHILD_HEAD + r'''
n = 4096
for curve in ("bls12_381", "bn254"):
    key = SK.halves(curve, n)
    half = SK.rand_scalars(curve, n // 2, 0xCAA0)
    cancel = half + half
    one_off = list(cancel)
    one_off[n // 2 + 1000] = (one_off[1000] + 77) % SK.modulus(curve)
    rnd = SK.rand_scalars(curve, n, 0xCAA1)
    srs = ctx.upload_srs(curve, key.bases)
    for table in (False, True):
        if table:
            srs.precompute(min_pairs=1)
        for name, s in (("random", rnd), ("cancel", cancel), ("one off", one_off), ("cancel", cancel)):
            want = SK.expected(key, s)
            assert want.any() == (name != "cancel")
            for arr, mont in ((SK.limbs(s), False), (SK.mont(curve, s), True)):
                got, inf = srs.msm(arr, montgomery=mont)
                assert (got == want).all() and inf == (not want.any()), (curve, table, name, mont)
    srs.free()
ctx.close()
print("parts ok")
'''


@pytest.mark.parametrize("parts", ["2", "4"])
def test_host_scalars_in_parts_whose_merges_cancel(parts):
    """pc_hip_msm on HOST scalars in parts (PC_HIP_HOST_SPLIT_LOG2 = 10, PC_HIP_HOST_PARTS = 2, 4; read once per process: a child),
    n = 4096 on halves(n) with s[j] = s[j + n / 2]: every bucket of the second half is the negative of the first half's, so
    BucketMergeBody adds P and -P in every bucket that is hit (two parts: every merge; four: the last one, after merges that do not
    cancel) and the MSM is the point at infinity; one scalar changed: the known point.  Table-free and over the window table, on
    BLS12-381 and BN254."""
    env = dict(os.environ, PC_HIP_HOST_SPLIT_LOG2="10", PC_HIP_HOST_PARTS=parts)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD_PARTS], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "parts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_msm_many_randomised_differential():
    """tools/msm_many_fuzz.py for ten seconds on all four curves.  FUZZ_MIN_CASES completed cases at least, so that a slice that ran
    almost nothing fails: at most half of the smaller of the two measured ten-second counts (the tool's docstring has both)."""
    import re
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "msm_many_fuzz.py"), "10", "20261020"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    found = re.search(r"msm_many_fuzz: (\d+) cases, 0 mismatches", r.stdout)
    assert found, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-1])
    assert int(found.group(1)) >= FUZZ_MIN_CASES


FUZZ_MIN_CASES = 75
