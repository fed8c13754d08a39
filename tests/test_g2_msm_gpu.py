"""pc_hip_g2_msm on the device against the pure-Python reference tests/harness/g2ref.py, bit-exact on the affine Montgomery bytes:
sizes around the window-width and chunk thresholds, both scalar forms, both memory sides, a base offset, adversarial scalar sets, a
2^20-pair call over a periodic key, and the residency accounting of G2 keys."""
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
