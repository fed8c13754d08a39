"""pc_hip_g2_msm on the device against the pure-Python reference tests/harness/g2ref.py, bit-exact on the affine Montgomery bytes:
sizes around the window-width and chunk thresholds, both scalar forms, both memory sides, a base offset, adversarial scalar sets, a
2^20-pair call over a periodic key, and the residency accounting of G2 keys; under the context's tuning knobs (window widths, chunks of
1 .. 64 entries) the joins of cut buckets at the 128-lane workgroup, equal and cancelling partial sums in those joins, an MSM whose sum
is the identity, 2^16 + 1 pairs, one MultilinearPC opening, and a ten-second slice of tools/g2_msm_fuzz.py."""
import numpy as np
import pytest

from harness import g2ref as G

pytestmark = pytest.mark.gpu
CURVE = "bls12_381"
NKEY = 4100


@pytest.fixture(scope="module")
def key_pts():
    ks = [(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % G.R for i in range(NKEY)]
    return G.fixed_base(G.generator()).mul_many(ks)


@pytest.fixture(scope="module")
def key(ctx, key_pts):
    k = ctx.upload_g2_srs(CURVE, G.points_array(key_pts))
    yield k
    k.free()


def rand_scalars(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(n)]


def check(got, want):
    out, inf = got
    assert G.point_from_bytes(out.tobytes()) == want
    assert inf == (want is G.INF)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1023, (1 << 12) + 1])
def test_g2_msm_sizes_forms_sides_offset(ctx, key, key_pts, n):
    import torch
    ks = rand_scalars(n, n)
    want = G.msm(key_pts[:n], ks)
    can, mont = G.scalars_array(ks, False), G.scalars_array(ks, True)
    check(key.msm(can), want)                                                    # canonical, host
    check(key.msm(mont, montgomery=True), want)                                  # Montgomery, host
    d_can, d_mont = torch.from_numpy(can).cuda(), torch.from_numpy(mont).cuda()
    check(key.msm(d_can, n=n), want)                                             # canonical, device
    check(key.msm(d_mont, n=n, montgomery=True), want)                           # Montgomery, device
    off = 3
    want_off = G.msm(key_pts[off:off + n], ks)
    check(key.msm(mont, montgomery=True, base_offset=off), want_off)
    check(key.msm(d_can, n=n, base_offset=off), want_off)
    # msm_bigint's truncation: more scalars than bases behind the offset
    tail = NKEY - 5
    check(key.msm(can, base_offset=tail), G.msm(key_pts[tail:], ks))


def test_g2_msm_adversarial_scalars(ctx, key_pts):
    n = 300
    b = list(key_pts[:n])
    b[5] = G.INF              # infinity among the bases
    b[11] = b[10]             # repeated base: a doubling inside a bucket
    k = ctx.upload_g2_srs(CURVE, G.points_array(b))
    rk = rand_scalars(3, n)
    cases = {
        "zeros": [0] * n,
        "ones": [1] * n,
        "r-1": [G.R - 1] * n,
        "same": [rk[0]] * n,
        "two-values": [rk[i % 2] for i in range(n)],
        "carry-chain": [((1 << 254) - 1 - i) % G.R for i in range(n)],
        "sparse": [rk[i] if i % 7 == 0 else 0 for i in range(n)],
    }
    try:
        for name, ks in cases.items():
            want = G.msm(b, ks)
            out, inf = k.msm(G.scalars_array(ks, False))
            assert G.point_from_bytes(out.tobytes()) == want and inf == (want is G.INF), name
            out, _ = k.msm(G.scalars_array(ks, True), montgomery=True)
            assert G.point_from_bytes(out.tobytes()) == want, name
    finally:
        k.free()


def test_g2_msm_2p20_on_a_periodic_key(ctx, key_pts):
    """H[x] = pool[x mod 1024]: repeated bases are legal input and stress huge buckets and the joins.  The expected point is the
    1024-point Python MSM of the scalars summed per residue."""
    n, m = 1 << 20, 1024
    pool = key_pts[:m]
    bases = np.ascontiguousarray(np.tile(G.points_array(pool), (n // m, 1)))
    rnd = np.random.RandomState(20)
    sc = np.frombuffer(rnd.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    sc[:, 31] &= 0x3f                                                           # canonical: below 2^254 < r
    sc[7] = 0
    vals = [int.from_bytes(row.tobytes(), "little") for row in sc]
    per = [0] * m
    for x, v in enumerate(vals):
        per[x % m] += v
    want = G.msm(pool, [v % G.R for v in per])
    k = ctx.upload_g2_srs(CURVE, bases)
    try:
        out, inf = k.msm(sc)
        assert G.point_from_bytes(out.tobytes()) == want and not inf
    finally:
        k.free()


# ---- the joins, the tunings and the cancelling sums ----------------------------------------------------------------------------
# A G2 key's pipeline is made at its first MSM (g2_lane), not at upload, and takes the context's tuning then: every test below sets
# the tuning before the upload, keeps it until the key is freed and resets it in `finally`.  The window width of a call is read
# back (last_msm_shape); the chunk length is not part of that shape: that it takes effect rests on reading MsmPlan::part_body,
# where cfg_.T goes straight into g.T.

POOL = 256


@pytest.fixture(scope="module")
def pool(key_pts):
    """the 256 points of the periodic keys: with runs of equal scalars, the infinity, the repeated point and the P / -P pair bring
    skipped entries, doublings and cancellations into the buckets"""
    p = list(key_pts[:POOL])
    p[5] = G.INF
    p[11] = p[10]
    p[21] = G.neg(p[20])
    return p


def periodic_bases(pool, n):
    m = len(pool)
    return np.ascontiguousarray(np.tile(G.points_array(pool), ((n + m - 1) // m, 1))[:n])


def periodic_want(pool, scalars):
    """the MSM over H[x] = pool[x mod len(pool)]: one len(pool)-point Python MSM of the scalars summed per residue, mod r (every
    pool point lies in the subgroup of order r)"""
    m = len(pool)
    per = [0] * m
    for x, v in enumerate(scalars):
        per[x % m] += v
    return G.msm(pool, [v % G.R for v in per])


def ints_of(arr):
    return [int.from_bytes(row.tobytes(), "little") for row in arr]


def canonical_bytes(seed, n):
    rnd = np.random.RandomState(seed)
    sc = np.frombuffer(rnd.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    sc[:, 31] &= 0x3f                                                           # canonical: below 2^254 < r
    return sc


def distributions(sc):
    """scalar sets whose buckets span a few lanes, a whole workgroup (128 lanes for G2), several workgroups"""
    n = len(sc)
    idx = np.arange(n)
    return {
        "uniform": sc,
        "five_values": np.ascontiguousarray(sc[idx % 5]),
        "all_equal": np.ascontiguousarray(np.repeat(sc[:1], n, axis=0)),
        "runs": np.ascontiguousarray(sc[idx // 300]),
        "sparse": np.ascontiguousarray(np.where((idx % 13 == 0)[:, None], sc, 0).astype(np.uint8)),
        "wg_runs": np.ascontiguousarray(sc[idx // 128]),                        # at T = 1: buckets of whole 128-lane workgroups
    }


def assert_identity(got, what):
    out, inf = got
    assert inf and not out.any(), what


@pytest.mark.parametrize("n", [700, 5000, 1 << 15])
def test_g2_msm_chains_of_cut_buckets(ctx, pool, n):
    """The joins of buckets that chunk edges cut -- k_accumulate's in-workgroup scan over 128 lanes, k_accumulate_edges across
    workgroups, the segmented reduction behind them -- on G2 points, as test_te_msm_chains_of_cut_buckets does it: chunks of 1, 2, 5
    and 8 entries (the automatic chunk is never shorter than 8) on the periodic key pool[x mod 256].  (That the chunk length takes
    effect is read from the code, see above: the shape of a call does not report it.)"""
    bases = periodic_bases(pool, n)
    dists = distributions(canonical_bytes(0xC4A1 + n, n))
    wants = {name: periodic_want(pool, ints_of(a)) for name, a in dists.items()}
    try:
        for T in (1, 2, 5, 8):
            ctx.set_msm_tuning(0, T)
            k = ctx.upload_g2_srs(CURVE, bases)
            try:
                for name, a in dists.items():
                    check(k.msm(a), wants[name])
            finally:
                k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("c,T", [(4, 1), (7, 3), (10, 16), (13, 64), (16, 0)])
def test_g2_msm_tunings(ctx, pool, c, T):
    """window widths and chunk lengths as test_msm_tunings sets them; the width is read back from the call's shape (the chunk length
    is not part of it: see above)"""
    n = 5000
    ks = rand_scalars(1234, n)
    want = periodic_want(pool, ks)
    ctx.set_msm_tuning(c, T)
    try:
        k = ctx.upload_g2_srs(CURVE, periodic_bases(pool, n))
        try:
            check(k.msm(G.scalars_array(ks, False)), want)
            assert ctx.last_msm_shape()["window_bits"] == c
            assert not ctx.last_msm_shape()["window_table"]
        finally:
            k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("n,T", [(64, 0), (4096, 0), (4096, 2), (5000, 5), (1 << 15, 0)])
def test_g2_msm_equal_partial_sums_meet_in_the_joins(ctx, key_pts, n, T):
    """ONE base under ONE scalar, as test_msm_equal_partial_sums_meet_in_the_joins: every chunk of a bucket's run sums to the same
    point, so the scan of k_accumulate, the edge kernel, the segmented and the bucket reduction add EQUAL partial sums and XyzzD::add
    takes its doubling branch over Fq2.  (Chunk length: see above.)"""
    base = key_pts[2]
    ctx.set_msm_tuning(0, T)
    try:
        k = ctx.upload_g2_srs(CURVE, np.ascontiguousarray(np.repeat(G.points_array([base]), n, axis=0)))
        try:
            for s in (rand_scalars(5, 1)[0], 1, 3):
                check(k.msm(G.scalars_array([s] * n, False)), G.mul(n * s % G.R, base))
        finally:
            k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


def cancelling_layouts(n):
    """index -> True where the base is -P: the first half P and the second half -P; P and -P alternating"""
    return {"halves": [i >= n // 2 for i in range(n)], "alternating": [bool(i & 1) for i in range(n)]}


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("n", [256, 4096, 5000])
def test_g2_msm_partial_sums_cancel_in_the_joins(ctx, key_pts, n, T):
    """n/2 times P and n/2 times -P under ONE scalar k: every bucket that is hit holds as many P as -P, and the MSM is the identity
    (the flag is set and the 192 bytes are zero).  With one -P turned into P it is 2k P.
    The device's sort does not keep index order inside a bucket (msm_sort.hpp: the coarse scatter and the fine pass place entries
    with LDS atomics; blocks of 2048 scalars stay in order, the entries of one block only roughly), so which join meets which pair
    is a matter of the layout only in the large:
      halves       a bucket's run is (about) all P, then all -P: lanes, the scan of a workgroup and whole workgroups hold
                   NON-TRIVIAL partial sums j k P that cancel against -j k P further right -- in the scan, in k_accumulate_edges
                   and in the segmented reduction; at n = 4096 the two halves are the two sort blocks, so the run is exactly that
      alternating  neighbours cancel: with an even chunk length most lanes' OWN partial sums are infinity (where the sort kept the
                   order), with an odd one they are +-k P and cancel pairwise in the first step of the scan.
    (Chunk length: see above.)"""
    P = key_pts[7]
    s = rand_scalars(21, 1)[0]
    sc = G.scalars_array([s] * n, False)
    pn = G.points_array([P, G.neg(P)])
    mixed = rand_scalars(22 + n, n)
    ctx.set_msm_tuning(0, T)
    try:
        for name, minus in cancelling_layouts(n).items():
            sel = np.array(minus, dtype=np.intp)
            k = ctx.upload_g2_srs(CURVE, np.ascontiguousarray(pn[sel]))
            try:
                # first a call with random scalars on the same pipeline: it leaves every partial-sum slot holding a point, so an
                # infinity that the next call does not WRITE to its slot would show
                signed = sum(-v if m else v for v, m in zip(mixed, minus))
                check(k.msm(G.scalars_array(mixed, False)), G.mul(signed % G.R, P))
                assert_identity(k.msm(sc), (name, n, T))
            finally:
                k.free()
            sel[[i for i in range(n) if minus[i]][n // 4]] = 0                      # one -P in the middle of them becomes P
            k = ctx.upload_g2_srs(CURVE, np.ascontiguousarray(pn[sel]))
            try:
                check(k.msm(sc), G.mul(2 * s % G.R, P))
            finally:
                k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


def test_g2_msm_whole_sum_is_the_identity(ctx, key_pts):
    """k P + (r - k) P + 7 (the all-zero entry) at the default tuning: the flag and the all-zero bytes, in both scalar forms, from host
    and from device scalars; then one scalar changed: a point again"""
    import torch
    n = 300
    b = list(key_pts[:n])
    b[5] = G.INF
    b[13] = b[12]
    ks = [0] * n
    ks[12], ks[13], ks[5] = 0x1234567, G.R - 0x1234567, 7
    assert G.msm(b, ks) is G.INF
    k = ctx.upload_g2_srs(CURVE, G.points_array(b))
    try:
        for mont in (False, True):
            a = G.scalars_array(ks, mont)
            assert_identity(k.msm(a, montgomery=mont), ("host", mont))
            assert_identity(k.msm(torch.from_numpy(a).cuda(), n=n, montgomery=mont), ("device", mont))
        ks[13] = G.R - 0x1234566
        out, inf = k.msm(G.scalars_array(ks, False))
        assert out.any() and not inf
        check((out, inf), G.msm(b, ks))
        assert G.msm(b, ks) == b[12]
    finally:
        k.free()


def test_g2_msm_2p16_plus_1_on_a_periodic_key(ctx, pool):
    """one pair more than 2^16, one zero scalar, default tuning: the reduction levels are cooperative from the first level on (the 2^20
    call above starts on the serial fan-in)"""
    n = (1 << 16) + 1
    sc = canonical_bytes(16, n)
    sc[7] = 0
    want = periodic_want(pool, ints_of(sc))
    k = ctx.upload_g2_srs(CURVE, periodic_bases(pool, n))
    try:
        out, inf = k.msm(sc)
        check((out, inf), want)
        assert not inf
    finally:
        k.free()


def test_ml_open_under_a_tuning(ctx):
    """One MultilinearPC opening, nv = 9, on a pair-sum key whose pipeline was made under (c, T) = (7, 3), equal to the reference's
    proof; and one call of round 0's length on the same key, whose shape shows the width the key's pipeline runs with (pc_hip_ml_open
    records none)."""
    import poly_commit_amd as pc
    nv, n = 9, 1 << 9
    rnd = np.random.RandomState(1900)
    rand_fr = lambda m: [int.from_bytes(rnd.bytes(32), "little") % G.R for _ in range(m)]
    t = rand_fr(nv)
    ck = G.ml_setup_with_trapdoor(nv, t)
    evals, point = rand_fr(n), rand_fr(nv)
    want = G.ml_open(ck, evals, point)
    ctx.set_msm_tuning(7, 3)
    try:
        key = pc.multilinear_pair_key(ctx, CURVE, [G.points_array(l) for l in ck["powers_of_h"]])
        try:
            out, inf = key.ml_open(G.scalars_array(evals, True), nv, G.scalars_array(point, True))
            assert [G.point_from_bytes(row.tobytes()) for row in out] == want and inf == [p is G.INF for p in want]
            q, _ = G.ml_fold(evals, point[0])
            check(key.msm(G.scalars_array(q, True), montgomery=True), want[0])
            assert ctx.last_msm_shape()["window_bits"] == 7
        finally:
            key.free()
    finally:
        ctx.set_msm_tuning(0, 0)


def _g2_fuzz(seconds, seed):
    import os, re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "g2_msm_fuzz.py"), seconds, seed], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"g2_msm_fuzz: (\d+) cases, 0 mismatches", r.stdout)
    assert m, r.stdout[-2000:]
    return int(m.group(1))


def test_g2_msm_randomised_differential():
    """tools/g2_msm_fuzz.py for ten seconds: random sizes, window widths, chunk lengths, distributions, scalar forms and base offsets on
    periodic G2 keys against g2ref.  At least 20 cases: the reference side alone manages several times that in ten seconds (the rate is
    in the tool's docstring), so a slice that ran almost nothing fails."""
    assert _g2_fuzz("10", "20261020") >= 20


def test_g2_key_residency(key_pts):
    import poly_commit_amd as pc
    c = pc.Context(0)
    before = c.bytes_resident()
    arr = G.points_array(key_pts[:1000])
    k = c.upload_g2_srs(CURVE, arr)
    assert len(k) == 1000
    mid = c.bytes_resident()
    assert mid["n_keys"] == before["n_keys"] + 1
    assert mid["device_total"] >= before["device_total"] + 1000 * 192
    assert k.bytes_resident()["bases"] == 1000 * 192 and k.bytes_resident()["lanes"] == 0
    out, _ = k.msm(G.scalars_array([1] * 10, False))
    assert k.bytes_resident()["lanes"] > 0                                       # the pipeline's workspace, created on first use
    assert c.bytes_resident()["device_total"] >= mid["device_total"] + k.bytes_resident()["lanes"]
    k.free()
    after = c.bytes_resident()
    assert after["n_keys"] == before["n_keys"] and after["device_total"] <= before["device_total"] + after["scratch"]
    # a key that was never freed goes with the context
    k2 = c.upload_g2_srs(CURVE, arr)
    assert c.bytes_resident()["n_keys"] == before["n_keys"] + 1
    c.close()
    c2 = pc.Context(0)
    assert c2.bytes_resident()["device_total"] <= before["device_total"]
    c2.close()
    k2.free()                                                                    # the handle only remains to be freed
