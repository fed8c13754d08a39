"""pc_hip_te_msm_many, pc_hip_te_fr_lincomb and pc_hip_te_fr_dot on the device, through the C ABI, against the pure-Python restatement
tests/harness/teref.py and Python integers: every row of a pass bit-exact on the affine Montgomery bytes, over the window table of a
key range -- shapes from one pair to 1025 x 1024, both scalar forms and memory sides, a base offset, low-order bases and rows that are
or cancel to the identity, one bucket cut across many lanes, the table's cache (another shape, a folded key) and its accounting, and
the argument checks that test_msm_many_and_precompute_argument_errors pins for G1."""
import ctypes as C

import numpy as np
import pytest

from harness import teref as E

pytestmark = pytest.mark.gpu
CURVE = "ed_on_bls12_381"
NKEY = 1100


def key_scalars(n):
    return [(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % E.R for i in range(n)]


@pytest.fixture(scope="module")
def key_pts():
    """1100 points, known multiples of G"""
    return E.fixed_base(E.GEN).mul_many(key_scalars(NKEY))


@pytest.fixture(scope="module")
def key(ctx, key_pts):
    k = ctx.upload_te_srs(CURVE, E.points_array(key_pts))
    yield k
    k.free()


def rand_scalars(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


def rows_array(rows, mont):
    B, m = len(rows), len(rows[0])
    return E.scalars_array([k for r in rows for k in r], mont).reshape(B, m, 32)


def check_rows(got, wants):
    out, ident = got
    assert out.shape == (len(wants), 64)
    for k, want in enumerate(wants):
        assert E.point_from_bytes(out[k].tobytes()) == want, k
        assert bool(ident[k]) == (want == E.IDENT), k
        if want == E.IDENT:
            assert out[k].tobytes() == E.IDENT_BYTES, k      # (0, ONE), never zeros


@pytest.mark.parametrize("m,B", [(1, 1), (1, 5), (2, 3), (33, 32), (65, 64), (64, 3)])
def test_te_msm_many_shapes_forms_sides_offset(ctx, key, key_pts, m, B):
    import torch
    rows = [rand_scalars(1000 * m + k, m) for k in range(B)]
    off = 7
    wants = [E.msm(key_pts[:m], r) for r in rows]
    wants_off = [E.msm(key_pts[off:off + m], r) for r in rows]
    can, mont = rows_array(rows, False), rows_array(rows, True)
    check_rows(key.msm_many(can), wants)                                                         # canonical, host
    check_rows(key.msm_many(mont, montgomery=True, base_offset=off), wants_off)                  # Montgomery, host, at an offset
    d_can, d_mont = torch.from_numpy(can).cuda(), torch.from_numpy(mont).cuda()
    check_rows(key.msm_many(d_mont, m=m, n_msms=B, montgomery=True), wants)                      # Montgomery, device
    check_rows(key.msm_many(d_can, m=m, n_msms=B, base_offset=off), wants_off)                   # canonical, device, at an offset
    shape = ctx.last_msm_shape()
    assert shape["window_bits"] >= 8 and shape["window_table"]


def adversarial_bases(key_pts, n):
    """the set of test_te_msm_adversarial_bases_and_scalars"""
    b = list(key_pts[:n])
    b[3] = E.IDENT
    b[5] = E.ZERO
    b[7] = E.T2
    b[8] = E.T4
    b[9] = E.T8
    b[11] = E.neg(b[10])
    b[13] = b[12]
    for i in range(20, 40):
        b[i] = E.add(b[i], E.T8)
    return b


def test_te_msm_many_adversarial_bases_and_scalars(ctx, key_pts):
    """Low-order points, the identity, an all-zero entry, P beside -P and repeats as bases; 0, 1, r - 1 and 2^251 mixed with random
    scalars; an all-zero row and rows that cancel give (0, ONE) with flag 1.  Expected values are integer-exact."""
    m = 65
    b = adversarial_bases(key_pts, m)
    rk = rand_scalars(3, m)
    special = [0, 1, E.R - 1, 1 << 251]
    rows = [
        [special[j % 4] for j in range(m)],
        [0] * m,                                                                   # no non-zero digit: the bucket set stays empty
        [rk[j] if j % 3 else special[(j // 3) % 4] for j in range(m)],
        [E.R - 1] * m,
        [1] * m,
        [1 << 251] * m,
        rk,
    ]
    cancel = [0] * m                                                               # k P + k (-P) + 8 T8 + 4 T4 + 2 T2 + 5 (0, 1) + 7 (all-zero entry)
    cancel[10] = cancel[11] = 0x1234567
    cancel[9], cancel[8], cancel[7], cancel[3], cancel[5] = 8, 4, 2, 5, 7
    rows.append(cancel)
    cancel2 = [0] * m                                                              # k P + (r - k) P on the repeated point
    cancel2[12], cancel2[13] = rk[0], E.R - rk[0]
    rows.append(cancel2)
    almost = list(cancel)
    almost[9] = 7                                                                  # 7 T8 is not the identity
    rows.append(almost)
    wants = [E.msm(b, r) for r in rows]
    assert wants[1] == wants[7] == wants[8] == E.IDENT and wants[9] == E.mul(7, E.T8)
    assert E.mul(E.R - 1, b[20]) != E.neg(b[20])                                   # (r - 1) P is not -P outside the subgroup
    k = ctx.upload_te_srs(CURVE, E.points_array(b))
    try:
        check_rows(k.msm_many(rows_array(rows, False)), wants)
        check_rows(k.msm_many(rows_array(rows, True), montgomery=True), wants)
        zeros = [[0] * m for _ in range(len(rows))]                                # every bucket set empty
        check_rows(k.msm_many(rows_array(zeros, False)), [E.IDENT] * len(rows))
    finally:
        k.free()


POOL = 1024


def test_te_msm_many_one_bucket_cut_across_many_lanes(ctx, key_pts):
    """All scalars of a row equal, m = 5000, B = 3, on the periodic key pool[x mod 1024] (as test_te_msm_chains_of_cut_buckets): every
    window's digit is one value, so one bucket per row holds all 5000 entries of that window and is cut across many lanes."""
    m, B = 5000, 3
    pool = list(key_pts[:POOL])
    for i in range(0, POOL, 37):
        pool[i] = E.add(pool[i], E.T8)
    pool[500] = E.IDENT
    bases = np.ascontiguousarray(np.tile(E.points_array(pool), ((m + POOL - 1) // POOL, 1))[:m])
    vals = [rand_scalars(0xC4A1, 1)[0], E.R - 1, 0x55]
    wants = []
    for v in vals:
        per = [0] * POOL
        for x in range(m):
            per[x % POOL] += v                 # integers, NOT reduced modulo r: the pool has points outside the prime-order subgroup
        wants.append(E.msm(pool, per))
    k = ctx.upload_te_srs(CURVE, bases)
    try:
        check_rows(k.msm_many(rows_array([[v] * m for v in vals], False)), wants)
    finally:
        k.free()


def test_te_msm_many_1025_x_1024(ctx, key, key_pts):
    """The shape of a 20-variable Hyrax commit on a key with known logarithms: row i is (sum_j s_ij k_j) G by the fixed-base table."""
    m, B = 1025, 1024
    rnd = np.random.RandomState(1025)
    sc = np.frombuffer(rnd.bytes(32 * m * B), dtype=np.uint8).reshape(B, m, 32).copy()
    sc[:, :, 31] &= 0x07                                                           # canonical: below 2^251 < r
    sc[5] = 0                                                                      # an all-zero row among them
    kk = key_scalars(m)
    flat = sc.reshape(B * m, 32)
    logs = []
    for i in range(B):
        row = flat[i * m:(i + 1) * m]
        logs.append(sum(int.from_bytes(row[j].tobytes(), "little") * kk[j] for j in range(m)) % E.R)
    wants = E.fixed_base(E.GEN).mul_many(logs)
    assert wants[5] == E.IDENT
    check_rows(key.msm_many(sc), wants)


def test_te_msm_many_cache(ctx, key_pts):
    """The table and the pipeline are cached per shape: the same shape twice, another shape and the first again give the same bits;
    pc_hip_te_msm on the key is unchanged by a many-MSM; after pc_hip_te_ec_fold on the key the table is rebuilt from the folded
    points (the stale-table case)."""
    n = 64
    pts = list(key_pts[:n])
    k = ctx.upload_te_srs(CURVE, E.points_array(pts))
    try:
        rows = [rand_scalars(50 + i, 32) for i in range(4)]
        arr = rows_array(rows, False)
        wants = [E.msm(pts[:32], r) for r in rows]
        single = rand_scalars(99, n)
        s_before, _ = k.msm(E.scalars_array(single, False))
        got = k.msm_many(arr)
        check_rows(got, wants)
        first = got[0]
        again, _ = k.msm_many(arr)
        assert (again == first).all()
        other = [rand_scalars(70 + i, 16) for i in range(3)]
        check_rows(k.msm_many(rows_array(other, False), base_offset=5), [E.msm(pts[5:21], r) for r in other])
        back, _ = k.msm_many(arr)
        assert (back == first).all()
        s_after, _ = k.msm(E.scalars_array(single, False))
        assert (s_after == s_before).all() and E.point_from_bytes(s_after.tobytes()) == E.msm(pts, single)
        # the key's first 32 points change: a table kept from before would give the old sums
        u = rand_scalars(7, 1)[0]
        k.ec_fold(32, E.scalars_array([u], True)[0])
        folded = E.fold(pts, u)
        assert k.bytes_resident()["window_tables"] == 0                            # dropped with the fold
        got = k.msm_many(arr)
        check_rows(got, [E.msm(folded, r) for r in rows])
        assert not (got[0] == first).all()
    finally:
        k.free()


def test_te_msm_many_ledger(key_pts):
    """pc_hip_te_srs_bytes_resident reports the table in out[1] -- windows x m x 96 bytes -- and the pass's pipeline in out[3]; the
    context counts the table with its window tables; freeing the key gives everything back."""
    import poly_commit_amd as pc
    c = pc.Context(0)
    try:
        before = c.bytes_resident()
        k = c.upload_te_srs(CURVE, E.points_array(key_pts[:200]))
        assert k.bytes_resident()["window_tables"] == 0
        m, B = 100, 6
        rows = [rand_scalars(i, m) for i in range(B)]
        out, _ = k.msm_many(rows_array(rows, False), base_offset=50)
        assert E.point_from_bytes(out[B - 1].tobytes()) == E.msm(key_pts[50:150], rows[B - 1])
        shape = c.last_msm_shape()
        res = k.bytes_resident()
        assert res["window_tables"] == shape["digits_per_scalar"] * m * 96 and shape["digits_per_scalar"] == 252 // shape["window_bits"] + 1
        assert res["lanes"] > 0 and res["fold_table"] == 0 and res["bases"] == 200 * 96
        held = c.bytes_resident()
        assert held["window_tables"] == before["window_tables"] + res["window_tables"]
        assert held["device_total"] >= before["device_total"] + res["window_tables"] + res["lanes"]
        lanes_many = res["lanes"]
        k.msm(E.scalars_array(rows[0], False))                                     # the single MSM's pipeline comes on top
        assert k.bytes_resident()["lanes"] > lanes_many
        k.free()
        after = c.bytes_resident()
        assert after["n_keys"] == before["n_keys"] and after["window_tables"] == before["window_tables"]
        assert after["device_total"] <= before["device_total"] + after["scratch"]
    finally:
        c.close()


def test_te_msm_many_argument_errors(ctx, key):
    """The codes test_msm_many_and_precompute_argument_errors pins for G1: negative status, nothing computed."""
    lib, vp = ctx.lib, C.c_void_p
    s = E.scalars_array(rand_scalars(3, 64), False)
    out = np.zeros((2, 64), dtype=np.uint8)
    INVALID, TOO_LARGE = -1, -5
    # bases[base_offset + m) must lie inside the key
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, NKEY - 4, vp(s.ctypes.data), 0, 0, 8, 2, vp(out.ctypes.data), None) == INVALID
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, NKEY + 1, vp(s.ctypes.data), 0, 0, 0, 2, vp(out.ctypes.data), None) == INVALID
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, None, 0, 0, 8, 2, vp(out.ctypes.data), None) == INVALID
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, vp(s.ctypes.data), 0, 0, 8, 2, None, None) == INVALID
    assert lib.pc_hip_te_msm_many(None, key.h, 0, vp(s.ctypes.data), 0, 0, 8, 2, vp(out.ctypes.data), None) == INVALID
    assert lib.pc_hip_te_msm_many(ctx.h, None, 0, vp(s.ctypes.data), 0, 0, 8, 2, vp(out.ctypes.data), None) == INVALID
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, vp(s.ctypes.data), 7, 0, 8, 2, vp(out.ctypes.data), None) == INVALID      # scalar form
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, vp(s.ctypes.data), 0, 7, 8, 2, vp(out.ctypes.data), None) == INVALID      # memory side
    # a key of another context
    import poly_commit_amd as pc
    c2 = pc.Context(0)
    try:
        assert lib.pc_hip_te_msm_many(c2.h, key.h, 0, vp(s.ctypes.data), 0, 0, 8, 2, vp(out.ctypes.data), None) == INVALID
    finally:
        c2.close()
    assert not out.any()
    # too many entries for the 31-bit entry index, too many buckets: PC_ERR_TOO_LARGE, before any allocation
    held, table = ctx.bytes_resident()["device_total"], key.bytes_resident()["window_tables"]      # (the key may hold an earlier test's table)
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, vp(s.ctypes.data), 0, 0, 64, 1 << 26, vp(out.ctypes.data), None) == TOO_LARGE
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, vp(s.ctypes.data), 0, 0, 1, 1 << 24, vp(out.ctypes.data), None) == TOO_LARGE
    assert ctx.bytes_resident()["device_total"] == held and key.bytes_resident()["window_tables"] == table
    # zero MSMs / zero pairs are fine
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, vp(s.ctypes.data), 0, 0, 8, 0, vp(out.ctypes.data), None) == 0
    assert not out.any()
    ident = (C.c_int * 2)()
    assert lib.pc_hip_te_msm_many(ctx.h, key.h, 0, None, 0, 0, 0, 2, vp(out.ctypes.data), ident) == 0
    assert list(ident) == [1, 1] and out[0].tobytes() == out[1].tobytes() == E.IDENT_BYTES


# ---- the vectors of Hyrax's opening over the 252-bit scalar field ----------------------------------------------------------------

def fr_ints(arr):
    ri = pow(E.MONT_R, -1, E.R)
    return [int.from_bytes(row.tobytes(), "little") * ri % E.R for row in arr.reshape(-1, 32)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_te_fr_dot_and_lincomb(ctx, n):
    """<a, b> and sum_j xi[j] v_j against Python integers: coefficients 0, 1 and r - 1 beside random ones, ragged lengths (a shorter
    vector counts as zero beyond its end), k = 0 (the zero vector), host and device vectors."""
    import torch
    a, b = rand_scalars(n, n), rand_scalars(n + 1, n)
    a[0] = E.R - 1
    if n > 2:
        b[1], a[2] = 0, 1
    am, bm = E.scalars_array(a, True), E.scalars_array(b, True)
    da, db = torch.from_numpy(am).cuda(), torch.from_numpy(bm).cuda()
    assert fr_ints(ctx.te_fr_dot(CURVE, da, db, n)) == [sum(x * y for x, y in zip(a, b)) % E.R]
    assert fr_ints(ctx.te_fr_dot(CURVE, da, da, n)) == [sum(x * x for x in a) % E.R]
    # five vectors of ragged lengths, coefficients 0, 1, r - 1 and two random ones
    lens = [n, max(1, n // 2), n, max(1, n - 1), 1]
    vecs = [rand_scalars(10 * n + j, lens[j]) for j in range(5)]
    xi = [0, 1, E.R - 1] + rand_scalars(n + 7, 2)
    want = [sum(xi[j] * vecs[j][i] for j in range(5) if i < lens[j]) % E.R for i in range(n)]
    host = [E.scalars_array(v, True) for v in vecs]
    xim = E.scalars_array(xi, True)
    assert fr_ints(ctx.te_fr_lincomb(CURVE, host, xim, n_out=n)) == want
    dev = [torch.from_numpy(h).cuda() for h in host]
    dout = torch.zeros((n, 32), dtype=torch.uint8).cuda()
    ctx.te_fr_lincomb(CURVE, dev, xim, n_out=n, out=dout, lens=lens)
    assert fr_ints(dout.cpu().numpy()) == want
    # n_out beyond every vector: zeros behind; k = 0: the zero vector
    longer = fr_ints(ctx.te_fr_lincomb(CURVE, host, xim, n_out=n + 3))
    assert longer == want + [0, 0, 0]
    none = ctx.te_fr_lincomb(CURVE, [], np.zeros((0, 32), dtype=np.uint8), n_out=n, out=np.full((n, 32), 0xff, dtype=np.uint8))
    assert not none.any()


def test_te_fr_argument_errors(ctx):
    """the checks and codes of pc_hip_fr_lincomb and pc_hip_fr_dot, and an unknown pc_te_curve"""
    import torch
    lib, vp = ctx.lib, C.c_void_p
    v = torch.zeros((4, 32), dtype=torch.uint8).cuda()
    out = np.zeros(32, dtype=np.uint8)
    INVALID, TOO_LARGE = -1, -5
    assert lib.pc_hip_te_fr_dot(None, 0, vp(v.data_ptr()), vp(v.data_ptr()), 4, vp(out.ctypes.data)) == INVALID
    assert lib.pc_hip_te_fr_dot(ctx.h, 1, vp(v.data_ptr()), vp(v.data_ptr()), 4, vp(out.ctypes.data)) == INVALID
    assert lib.pc_hip_te_fr_dot(ctx.h, 0, None, vp(v.data_ptr()), 4, vp(out.ctypes.data)) == INVALID
    assert lib.pc_hip_te_fr_dot(ctx.h, 0, vp(v.data_ptr()), vp(v.data_ptr()), 4, None) == INVALID
    assert lib.pc_hip_te_fr_dot(ctx.h, 0, vp(v.data_ptr()), vp(v.data_ptr()), 1 << 32, vp(out.ctypes.data)) == TOO_LARGE
    assert lib.pc_hip_te_fr_dot(ctx.h, 0, None, None, 0, vp(out.ctypes.data)) == 0 and not out.any()      # the empty product
    polys = (C.c_void_p * 1)(v.data_ptr())
    lens = (C.c_size_t * 1)(4)
    xi = E.scalars_array([1], True)
    o4 = np.zeros((4, 32), dtype=np.uint8)
    assert lib.pc_hip_te_fr_lincomb(None, 0, polys, 1, lens, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 2, polys, 1, lens, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, None, 1, lens, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, polys, 1, None, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, polys, 1, lens, 1, None, vp(o4.ctypes.data), 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, polys, 1, lens, 1, vp(xi.ctypes.data), None, 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, polys, 1, lens, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 1 << 32) == TOO_LARGE
    big = (C.c_size_t * 1)(1 << 32)
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, polys, 1, big, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 4) == TOO_LARGE
    null_poly = (C.c_void_p * 1)(None)
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, null_poly, 1, lens, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 4) == INVALID
    assert lib.pc_hip_te_fr_lincomb(ctx.h, 0, polys, 1, lens, 1, vp(xi.ctypes.data), vp(o4.ctypes.data), 0, 0) == 0
