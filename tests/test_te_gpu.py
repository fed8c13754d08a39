"""pc_hip_te_msm and pc_hip_te_ec_fold on the device against the pure-Python restatement tests/harness/teref.py, bit-exact on the affine
Montgomery bytes: sizes around the window-width and chunk thresholds, both scalar forms, both memory sides, a base offset, bases of
low order and outside the prime-order subgroup crossed with adversarial scalar sets (expected values are integer-exact: a use of
r P = O anywhere in the pipeline shows here), an MSM whose sum is the identity, the joins of cut buckets under the tuning knobs on a
periodic key, the key fold with its special lanes, and the residency accounting of the typed key.
(Handle typing has no test: pc_te_srs is a distinct C type, which a ctypes call cannot express -- it would reinterpret the object.)"""
import numpy as np
import pytest

from harness import teref as E

pytestmark = pytest.mark.gpu
CURVE = "ed_on_bls12_381"
NKEY = 4100


def key_scalars(n):
    return [(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % E.R for i in range(n)]


@pytest.fixture(scope="module")
def key_pts():
    """about 4100 points, known multiples of G"""
    return E.fixed_base(E.GEN).mul_many(key_scalars(NKEY))


@pytest.fixture(scope="module")
def key(ctx, key_pts):
    k = ctx.upload_te_srs(CURVE, E.points_array(key_pts))
    yield k
    k.free()


def rand_scalars(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


def check(got, want):
    out, ident = got
    assert E.point_from_bytes(out.tobytes()) == want
    assert ident == (want == E.IDENT)
    if ident:
        assert out.tobytes() == E.IDENT_BYTES


def test_te_key_upload_and_read_back(ctx, key, key_pts):
    """read-back is the caller's x || y whatever the resident form; a strided host array is repacked"""
    assert len(key) == NKEY
    assert (key.read(0, 7) == E.points_array(key_pts[:7])).all()
    assert (key.read(NKEY - 3, 3) == E.points_array(key_pts[-3:])).all()
    wide = np.zeros((5, 80), dtype=np.uint8)
    wide[:, :64] = E.points_array(key_pts[10:15])
    wide[:, 64:] = 0xff
    k = ctx.upload_te_srs(CURVE, wide, stride_bytes=80)
    try:
        assert (k.read(0, 5) == E.points_array(key_pts[10:15])).all()
    finally:
        k.free()
    # points that already are on the device (packed), and an empty key
    import torch
    dev = torch.from_numpy(E.points_array(key_pts[20:52])).cuda()
    k = ctx.upload_te_srs(CURVE, dev, n=32)
    try:
        assert (k.read(0, 32) == E.points_array(key_pts[20:52])).all()
        ks = rand_scalars(5, 32)
        check(k.msm(E.scalars_array(ks, False)), E.msm(key_pts[20:52], ks))
    finally:
        k.free()
    k = ctx.upload_te_srs(CURVE, np.zeros((0, 64), dtype=np.uint8))
    try:
        assert len(k) == 0
        check(k.msm(np.zeros((0, 32), dtype=np.uint8)), E.IDENT)
    finally:
        k.free()


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1023, (1 << 12) + 1])
def test_te_msm_sizes_forms_sides_offset(ctx, key, key_pts, n):
    import torch
    ks = rand_scalars(n, n)
    want = E.msm(key_pts[:n], ks)
    can, mont = E.scalars_array(ks, False), E.scalars_array(ks, True)
    check(key.msm(can), want)                                                    # canonical, host
    check(key.msm(mont, montgomery=True), want)                                  # Montgomery, host
    d_can, d_mont = torch.from_numpy(can).cuda(), torch.from_numpy(mont).cuda()
    check(key.msm(d_can, n=n), want)                                             # canonical, device
    check(key.msm(d_mont, n=n, montgomery=True), want)                           # Montgomery, device
    off = 3
    want_off = E.msm(key_pts[off:off + n], ks)
    check(key.msm(mont, montgomery=True, base_offset=off), want_off)
    check(key.msm(d_can, n=n, base_offset=off), want_off)
    # msm_bigint's truncation: more scalars than bases behind the offset
    tail = NKEY - 5
    check(key.msm(can, base_offset=tail), E.msm(key_pts[tail:], ks))
    check(key.msm(can, base_offset=NKEY), E.IDENT)                               # nothing behind the offset: the empty sum


def adversarial_bases(key_pts, n):
    b = list(key_pts[:n])
    b[3] = E.IDENT                         # the identity (0, 1)
    b[5] = E.ZERO                          # an all-zero entry: not a curve point, counts as the identity
    b[7] = E.T2                            # (0, -1), order 2
    b[8] = E.T4                            # order 4
    b[9] = E.T8                            # order 8
    b[11] = E.neg(b[10])                   # P and -P side by side
    b[13] = b[12]                          # a repeated P
    for i in range(20, 40):                # twenty points outside the prime-order subgroup
        b[i] = E.add(b[i], E.T8)
    return b


def test_te_msm_adversarial_bases_and_scalars(ctx, key_pts):
    n = 300
    b = adversarial_bases(key_pts, n)
    assert all(E.on_curve(p) for p in b if p != E.ZERO)
    k = ctx.upload_te_srs(CURVE, E.points_array(b))
    rk = rand_scalars(3, n)
    cases = {
        "zeros": [0] * n,
        "ones": [1] * n,
        "r-1": [E.R - 1] * n,
        "same": [rk[0]] * n,
        "two-values": [rk[i % 2] for i in range(n)],
        "carry-chain": [((1 << 252) - 1 - i) % E.R for i in range(n)],
        "sparse": [rk[i] if i % 7 == 0 else 0 for i in range(n)],
    }
    try:
        for name, ks in cases.items():
            want = E.msm(b, ks)
            out, ident = k.msm(E.scalars_array(ks, False))
            assert E.point_from_bytes(out.tobytes()) == want and ident == (want == E.IDENT), name
            out, _ = k.msm(E.scalars_array(ks, True), montgomery=True)
            assert E.point_from_bytes(out.tobytes()) == want, name
        # (r - 1) times a point outside the subgroup is NOT its negative: the expected value above is integer-exact
        assert E.mul(E.R - 1, b[20]) != E.neg(b[20])
    finally:
        k.free()


def test_te_msm_whole_sum_is_the_identity(ctx, key_pts):
    """k P + (r - k) P + 8 T8 + 4 T4 + 2 T2 + 5 (0, 1) + 7 (all-zero entry): the flag and the (0, ONE) bytes"""
    n = 300
    b = adversarial_bases(key_pts, n)
    ks = [0] * n
    ks[12], ks[13], ks[9], ks[8], ks[7], ks[3], ks[5] = 0x1234567, E.R - 0x1234567, 8, 4, 2, 5, 7
    assert E.msm(b, ks) == E.IDENT
    k = ctx.upload_te_srs(CURVE, E.points_array(b))
    try:
        for mont in (False, True):
            out, ident = k.msm(E.scalars_array(ks, mont), montgomery=mont)
            assert ident and out.tobytes() == E.IDENT_BYTES
        ks[9] = 7                          # 7 T8 is not the identity
        out, ident = k.msm(E.scalars_array(ks, False))
        assert not ident and E.point_from_bytes(out.tobytes()) == E.mul(7, E.T8)
    finally:
        k.free()


POOL = 1024


@pytest.fixture(scope="module")
def pool(key_pts):
    """the 1024 points of the periodic keys: subgroup points, with an order-8 component on every 37th and the identity once"""
    p = list(key_pts[:POOL])
    for i in range(0, POOL, 37):
        p[i] = E.add(p[i], E.T8)
    p[500] = E.IDENT
    return p


def periodic_want(pool, scalars):
    per = [0] * POOL
    for x, v in enumerate(scalars):
        per[x % POOL] += v                 # integers, NOT reduced modulo r: the pool has points outside the prime-order subgroup
    return E.msm(pool, per)


def ints_of(arr):
    return [int.from_bytes(row.tobytes(), "little") for row in arr]


@pytest.mark.parametrize("n", [700, 5000, 1 << 15])
def test_te_msm_chains_of_cut_buckets(ctx, pool, n):
    """The joins of buckets that chunk edges cut (k_accumulate's in-workgroup scan, k_accumulate_edges, the segmented reduction
    behind them) under the context's tuning knobs, as test_msm_chains_of_cut_buckets does it: chunks of 1, 2, 5 and 8 entries against
    scalar distributions whose buckets span a few lanes, a whole workgroup, several workgroups, on the periodic key pool[x mod 1024]."""
    bases = np.ascontiguousarray(np.tile(E.points_array(pool), ((n + POOL - 1) // POOL, 1))[:n])
    rnd = np.random.RandomState(0xC4A1 + n)
    sc = np.frombuffer(rnd.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    sc[:, 31] &= 0x07                                                           # canonical: below 2^251 < r
    idx = np.arange(n)
    dists = {
        "uniform": sc,
        "five_values": np.ascontiguousarray(sc[idx % 5]),
        "all_equal": np.ascontiguousarray(np.repeat(sc[:1], n, axis=0)),
        "runs": np.ascontiguousarray(sc[idx // 300]),
        "sparse": np.ascontiguousarray(np.where((idx % 13 == 0)[:, None], sc, 0).astype(np.uint8)),
    }
    wants = {name: periodic_want(pool, ints_of(a)) for name, a in dists.items()}
    try:
        for T in (1, 2, 5, 8):
            ctx.set_msm_tuning(0, T)
            k = ctx.upload_te_srs(CURVE, bases)                                 # (the key's pipeline takes the tuning when it is made)
            try:
                for name, a in dists.items():
                    out, _ = k.msm(a)
                    assert E.point_from_bytes(out.tobytes()) == wants[name], (name, T, n)
            finally:
                k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


@pytest.mark.parametrize("c,T", [(4, 1), (7, 3), (10, 16), (13, 64), (16, 0)])
def test_te_msm_tunings(ctx, pool, c, T):
    """window widths and chunk lengths as test_msm_tunings sets them; the width is read back from the call's shape, so a tuning that
    was silently ignored fails here"""
    n = 5000
    bases = np.ascontiguousarray(np.tile(E.points_array(pool), (5, 1))[:n])
    ks = rand_scalars(1234, n)
    want = periodic_want(pool, ks)
    ctx.set_msm_tuning(c, T)
    try:
        k = ctx.upload_te_srs(CURVE, bases)
        try:
            out, _ = k.msm(E.scalars_array(ks, False))
            assert ctx.last_msm_shape()["window_bits"] == c
            assert E.point_from_bytes(out.tobytes()) == want
        finally:
            k.free()
    finally:
        ctx.set_msm_tuning(0, 0)


def test_te_msm_2p16_plus_1_on_a_periodic_key(ctx, pool):
    n = (1 << 16) + 1
    bases = np.ascontiguousarray(np.tile(E.points_array(pool), (n // POOL + 1, 1))[:n])
    rnd = np.random.RandomState(16)
    sc = np.frombuffer(rnd.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    sc[:, 31] &= 0x07
    sc[7] = 0
    want = periodic_want(pool, ints_of(sc))
    k = ctx.upload_te_srs(CURVE, bases)
    try:
        out, ident = k.msm(sc)
        assert E.point_from_bytes(out.tobytes()) == want and not ident
    finally:
        k.free()


@pytest.mark.parametrize("n_half", [1, 2, 63, 64, 65, 1000])
def test_te_ec_fold(ctx, key_pts, n_half):
    """key[i] = key[i] + u key[n_half + i] in place, for u = 0, 1, 2, r - 1 and a random one, with lanes whose left, right or both
    operands are the identity (or the all-zero entry), whose sum is a doubling or the identity, and with operands of low order; then an
    MSM over the folded key, which reads the rebuilt third coordinate."""
    fb = E.fixed_base(E.GEN)
    kk = key_scalars(2 * n_half)
    spare = key_pts[2100:2110]
    us = [0, 1, 2, E.R - 1, rand_scalars(n_half, 1)[0]]
    for u in us:
        pts = list(key_pts[:2 * n_half])
        special = {0: (E.IDENT, spare[0]), 1: (spare[1], E.IDENT), 2: (E.IDENT, E.IDENT), 3: (E.ZERO, E.ZERO),
                   4: (E.mul(u, spare[4]), spare[4]),                          # a doubling: left = u * right
                   5: (E.neg(E.mul(u, spare[5])), spare[5]),                   # the identity
                   6: (E.T8, spare[6]), 7: (spare[7], E.add(spare[8], E.T8)), 8: (E.T4, E.T2), 9: (E.ZERO, spare[9])}
        special = {i: lr for i, lr in special.items() if i < n_half}
        for i, (l, r) in special.items():
            pts[i], pts[n_half + i] = l, r
        # the ordinary lanes are known multiples of G: (k_i + u k_{half + i}) G by the fixed-base table
        want = fb.mul_many([(kk[i] + u * kk[n_half + i]) % E.R for i in range(n_half)])
        for i, (l, r) in special.items():
            want[i] = E.add(l, E.mul(u, r))
        if n_half > 5 and u:
            assert want[5] == E.IDENT and want[4] == E.mul(2, special[4][0])
        k = ctx.upload_te_srs(CURVE, E.points_array(pts))
        try:
            k.ec_fold(n_half, E.scalars_array([u], True)[0])
            assert len(k) == 2 * n_half
            got = k.read(0, n_half)
            assert [E.point_from_bytes(row.tobytes()) for row in got] == want, u
            assert (k.read(n_half, n_half) == E.points_array(pts[n_half:])).all()      # the upper half is left as it was
            m = max(1, n_half // 2)
            ks = rand_scalars(u % 1000 + n_half, m)
            out, _ = k.msm(E.scalars_array(ks, False), n=m, base_offset=0)
            assert E.point_from_bytes(out.tobytes()) == E.msm(want[:m], ks), u
        finally:
            k.free()


def test_te_ec_fold_argument_checks(ctx, key, key_pts):
    from poly_commit_amd import PcHipError
    u = E.scalars_array([3], True)[0]
    with pytest.raises(PcHipError):
        key.ec_fold(NKEY // 2 + 1, u)                                           # 2 n_half > len
    with pytest.raises(PcHipError):
        key.msm(E.scalars_array([1], False), base_offset=NKEY + 1)
    with pytest.raises(PcHipError):
        key.read(NKEY - 1, 2)
    with pytest.raises(PcHipError):
        ctx.upload_te_srs(CURVE, E.points_array([E.GEN]), stride_bytes=32)      # a stride below the point size
    key.ec_fold(0, u)                                                           # nothing to fold: the key is untouched
    assert (key.read(0, 2) == E.points_array(key_pts[:2])).all()


def test_te_key_residency(key_pts):
    """The accounting of test_g2_key_residency for the typed twisted Edwards key: the caller's points are 64 bytes; the key holds
    x || y || 2dxy, 96 bytes a point, and reports what it holds."""
    import poly_commit_amd as pc
    c = pc.Context(0)
    before = c.bytes_resident()
    arr = E.points_array(key_pts[:1000])
    k = c.upload_te_srs(CURVE, arr)
    assert len(k) == 1000
    mid = c.bytes_resident()
    assert mid["n_keys"] == before["n_keys"] + 1
    assert mid["device_total"] >= before["device_total"] + 1000 * 64
    assert k.bytes_resident()["bases"] == 1000 * 96 and k.bytes_resident()["lanes"] == 0
    assert k.bytes_resident()["window_tables"] == 0 and k.bytes_resident()["fold_table"] == 0
    out, _ = k.msm(E.scalars_array([1] * 10, False))
    assert E.point_from_bytes(out.tobytes()) == E.msm(key_pts[:10], [1] * 10)
    assert k.bytes_resident()["lanes"] > 0                                       # the pipeline's workspace, created on first use
    assert c.bytes_resident()["device_total"] >= mid["device_total"] + k.bytes_resident()["lanes"]
    k.free()
    after = c.bytes_resident()
    assert after["n_keys"] == before["n_keys"] and after["device_total"] <= before["device_total"] + after["scratch"]
    # a key that was never freed goes with the context
    k2 = c.upload_te_srs(CURVE, arr)
    assert c.bytes_resident()["n_keys"] == before["n_keys"] + 1
    c.close()
    c2 = pc.Context(0)
    assert c2.bytes_resident()["device_total"] <= before["device_total"]
    c2.close()
    k2.free()                                                                    # the handle only remains to be freed
