"""sample_generators over the short Weierstrass curves on the device: pc_hip_sample_generators bit for bit against the Python
restatement tests/harness/sw_setup.py -- points and digest counts, every curve, the wave / block / normalisation-tile edges, every
alignment of the counter behind the name, the counter's carry into its high word --, pc_hip_srs_prefix, the argument errors, and
poly_commit_amd/setup.py end to end: a Pallas IPA key made on the device, trimmed, committed to, opened and checked through ipa.py, and
a BLS12-377 Hyrax key through tests/harness/hyrax.py.

(PC_ERR_INTERNAL, a lane at the cap of 256 digests, cannot be reached through the ABI: Blake2s would have to reject 256 times in a row,
probability below 1e-23 per index.)"""
import ctypes as C

import numpy as np
import pytest

from harness import ref377
from harness import sw_setup as S

pytestmark = pytest.mark.gpu
R = S.R
CURVES = S.CURVES
NAME = S.IPA_NAME
INVALID_ARG, TOO_LARGE = -1, -5


def words_of(curve, pts):
    return np.array([S.point_words(curve, q) for q in pts], dtype=np.uint32)


def read_words(key, offset, count):
    return np.ascontiguousarray(key.read(offset, count)).view(np.uint32)


def sample(ctx, curve, name, first, count):
    """-> (point words, digest counts) of a generated key, read back and freed"""
    key, digests = ctx.sample_generators(curve, name, first, count, want_digests=True)
    try:
        assert key.n == count
        return read_words(key, 0, count), [int(x) for x in digests]
    finally:
        key.free()


def expect(curve, name, first, count):
    pts, counts = S.generators(curve, name, first, count)
    return words_of(curve, pts), counts


def same(got, want):
    return (got[0] == want[0]).all() and got[1] == want[1]


# ---- pc_hip_sample_generators ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("curve", CURVES)
def test_sample_generators_bit_exact(ctx, curve, count):
    """one lane, the wave edge, more than one block and more than one normalisation tile; the reference of the 1000 is shared"""
    assert same(sample(ctx, curve, NAME, 0, count), expect(curve, NAME, 0, count))


@pytest.mark.parametrize("name", [b"", NAME, S.HYRAX_NAME, bytes(range(1, 48)), bytes(range(1, 49))], ids=lambda n: "%d bytes" % len(n))
@pytest.mark.parametrize("curve", CURVES)
def test_name_lengths(ctx, curve, name):
    """0, 10, 14, 47 and 48 bytes: each alignment of the counter words; with 48 the retry message is exactly one 64-byte block"""
    got = sample(ctx, curve, name, 0, 8)
    assert same(got, expect(curve, name, 0, 8))
    assert max(got[1]) > 1, "none of the 8 indices retried"


@pytest.mark.parametrize("first", [0, 7, (1 << 32) - 3, (1 << 64) - 1000], ids=["0", "7", "2^32-3", "2^64-1000"])
@pytest.mark.parametrize("curve", CURVES)
def test_first_index(ctx, curve, first):
    """2^32 - 3 .. 2^32 + 2: the counter's carry into the high word"""
    assert same(sample(ctx, curve, NAME, first, 6), expect(curve, NAME, first, 6))


@pytest.mark.parametrize("curve", CURVES)
def test_adjacent_ranges_are_one_range(ctx, curve):
    a, c = 37, 63
    whole = sample(ctx, curve, NAME, 0, a + c)
    left, right = sample(ctx, curve, NAME, 0, a), sample(ctx, curve, NAME, a, c)
    assert (np.concatenate([left[0], right[0]]) == whole[0]).all() and left[1] + right[1] == whole[1]


def test_without_digest_counts(ctx):
    key = ctx.sample_generators("bn254", NAME, 0, 5)
    try:
        assert (read_words(key, 0, 5) == expect("bn254", NAME, 0, 5)[0]).all()
    finally:
        key.free()


@pytest.mark.parametrize("curve", CURVES)
def test_generated_key_commits(ctx, curve):
    """the key is a working pc_srs: an MSM over it with the scalars 1, 2, 3, .. is the sum the restatement gives"""
    n = 8
    key = ctx.sample_generators(curve, NAME, 0, n)
    try:
        scalars = ref377.limbs(list(range(1, n + 1)), 4)
        got, inf = key.msm(scalars)
        want = R.INF
        for k, q in enumerate(S.generators(curve, NAME, 0, n)[0]):
            want = R.ec_add(curve, want, S.mul(curve, k + 1, q))
        assert not inf and [int(w) for w in np.ascontiguousarray(got).view(np.uint32)] == S.point_words(curve, want)
    finally:
        key.free()


def raw_sample(ctx, curve, name, name_len, first, count):
    h = C.c_void_p()
    rc = ctx.lib.pc_hip_sample_generators(ctx.h, curve, name, name_len, first, count, None, C.byref(h))
    assert h.value is None or rc == 0
    return rc, h


def test_argument_errors(ctx):
    ctx.sample_generators("bls12_381", NAME, 0, 8).free()                          # the context's grow-only workspace is there before the count
    before = ctx.bytes_resident()
    assert raw_sample(ctx, 0, bytes(49), 49, 0, 4)[0] == INVALID_ARG               # the name is too long
    assert raw_sample(ctx, 0, NAME, len(NAME), 0, 0)[0] == INVALID_ARG             # no generators
    assert raw_sample(ctx, 0, NAME, len(NAME), (1 << 64) - 3, 4)[0] == INVALID_ARG  # first_index + count leaves 64 bits
    for curve in (4, 17, -1):
        assert raw_sample(ctx, curve, NAME, len(NAME), 0, 4)[0] == INVALID_ARG
    for count in (1 << 31, 1 << 40):
        assert raw_sample(ctx, 2, NAME, len(NAME), 0, count)[0] == TOO_LARGE
    rc, h = raw_sample(ctx, 2, NAME, len(NAME), (1 << 64) - 5, 4)                   # the last four indices that fit
    assert rc == 0
    ctx.lib.pc_hip_srs_free(h)
    key = ctx.sample_generators("pallas", NAME, 0, 8)
    try:
        for count in (0, 9):
            out = C.c_void_p()
            assert ctx.lib.pc_hip_srs_prefix(ctx.h, key.h, count, C.byref(out)) == INVALID_ARG and out.value is None
    finally:
        key.free()
    after = ctx.bytes_resident()
    assert (after["device_total"], after["n_keys"]) == (before["device_total"], before["n_keys"])      # no refused call left a key behind


# ---- pc_hip_srs_prefix ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", ["bls12_381", "pallas"])
def test_prefix(ctx, curve):
    n = 100
    key = ctx.sample_generators(curve, NAME, 0, n)
    try:
        key.precompute()                                                         # the source has a window table; the prefix must not
        whole = read_words(key, 0, n)
        assert (whole == expect(curve, NAME, 0, n)[0]).all()
        for count in (1, 64, n):
            pre = key.prefix(count)
            try:
                assert pre.n == count and (read_words(pre, 0, count) == whole[:count]).all()
                res = pre.bytes_resident()
                assert res["bases"] == count * whole.shape[1] * 4 and res["window_tables"] == 0 and res["fold_table"] == 0
                assert pre.fold_table_info() == (0, 0)
            finally:
                pre.free()
        assert (read_words(key, 0, n) == whole).all() and key.n == n             # the source is unchanged
        assert key.bytes_resident()["window_tables"] > 0
    finally:
        key.free()


# ---- setup, trim, commit, open, check -------------------------------------------------------------------------------------------------

def fr_mont(curve, vals):
    r = R.curve_params(curve)[1]
    return ref377.limbs([v % r * (1 << 256) % r for v in vals], 4)


def test_pallas_ipa_setup_trim_commit_open_check(ctx):
    import torch
    from poly_commit_amd import ipa
    from poly_commit_amd import setup as D
    curve = "pallas"
    r = R.curve_params(curve)[1]
    pp = D.ipa_setup(ctx, curve, (1 << 10) - 1)
    ck = None
    try:
        want = S.ipa_setup(curve, (1 << 10) - 1)
        assert pp["max_degree"] == 1023 and pp["comm_key"].n == 1024
        assert (read_words(pp["comm_key"], 0, 1024) == words_of(curve, want["comm_key"])).all()
        assert [int(w) for w in pp["s"].view(np.uint32)] == S.point_words(curve, want["s"])
        assert [int(w) for w in pp["h"].view(np.uint32)] == S.point_words(curve, want["h"])
        with pytest.raises(ValueError, match="TrimmingDegreeTooLarge"):
            D.ipa_trim(pp, 1024)
        ck = D.ipa_trim(pp, 300)
        n = 512
        assert ck["comm_key"].n == n and ck["supported_degree"] == n - 1 and pp["comm_key"].n == 1024
        rnd = np.random.RandomState(1313)
        coeffs = [int.from_bytes(rnd.bytes(32), "little") % r for _ in range(n)]
        z, xi = (int.from_bytes(rnd.bytes(32), "little") % r for _ in range(2))
        value = 0
        for c_ in reversed(coeffs):
            value = (value * z + c_) % r
        cdev = torch.from_numpy(fr_mont(curve, coeffs).view(np.int64)).cuda()
        comm, inf = ck["comm_key"].msm(cdev.data_ptr(), n=n, montgomery=True)
        assert not inf
        point, xis, values = fr_mont(curve, [z])[0], fr_mont(curve, [xi]), fr_mont(curve, [value])
        (l, rr, fk, c), _ = ipa.ipa_open(ctx, curve, ck["comm_key"], ck["h"], [cdev.data_ptr()], [n], [comm], point, xis)
        assert len(l) == 9 and len(rr) == 9
        assert (read_words(ck["comm_key"], 0, 8) == words_of(curve, want["comm_key"][:8])).all()      # the opening left the key alone
        assert ipa.ipa_check(ctx, curve, ck["comm_key"], ck["h"], [comm], point, values, (l, rr, fk, c), xis) is True
        bad = np.array(c, copy=True)
        bad.view(np.uint8)[0] ^= 1                                                                    # one flipped proof byte
        assert ipa.ipa_check(ctx, curve, ck["comm_key"], ck["h"], [comm], point, values, (l, rr, fk, bad), xis) is False
    finally:
        if ck is not None:
            ck["comm_key"].free()
        pp["comm_key"].free()


def test_bls12_377_hyrax_setup_commit_open_check(ctx):
    import torch
    from harness import hyrax
    from poly_commit_amd import setup as D
    curve, num_vars = "bls12_377", 4
    for bad in (None, 3):
        with pytest.raises(ValueError, match="InvalidNumberOfVariables"):
            D.hyrax_setup(ctx, curve, bad)
    pp = D.hyrax_setup(ctx, curve, num_vars)
    want = S.hyrax_setup(curve, num_vars)
    dim = 4
    assert pp["com_key"].shape == (dim, 12)
    assert (np.ascontiguousarray(pp["com_key"]).view(np.uint32) == words_of(curve, want["com_key"])).all()
    assert [int(w) for w in pp["h"].view(np.uint32)] == S.point_words(curve, want["h"])
    fr = R.CURVES[curve]["fr"]
    evals, rands, point = R.gen_scalars(fr, 0x771, 1 << num_vars), R.gen_scalars(fr, 0x772, dim), R.gen_scalars(fr, 0x773, num_vars)
    rnd, c = R.gen_scalars(fr, 0x774, dim + 3), R.gen_scalars(fr, 0x775, 1)[0]
    want_rows, mat_i = R.hyrax_commit(curve, want["com_key"], want["h"], evals, rands)
    want_proof, want_eval = R.hyrax_open(curve, want["com_key"], want["h"], mat_i, rands, point, rnd[0], rnd[1:1 + dim], rnd[1 + dim], rnd[2 + dim], c)
    assert R.hyrax_check(curve, want["com_key"], want["h"], want_rows, point, want_proof, c) is True
    m = lambda v: fr_mont(curve, v)                                  # noqa: E731
    key = hyrax.HyraxKey(ctx, curve, pp["com_key"], pp["h"])
    try:
        ev_dev = torch.from_numpy(m(evals).view(np.int64)).cuda()
        row_coms, state = hyrax.commit(key, ev_dev, m(rands))
        assert (np.ascontiguousarray(row_coms).view(np.uint32) == words_of(curve, want_rows)).all()
        proof, ev = hyrax.open(key, state, m(point), m([rnd[0]])[0], m(rnd[1:1 + dim]), m([rnd[1 + dim]])[0], m([rnd[2 + dim]])[0], m([c])[0])
        assert ref377.fr_from_mont(ev.reshape(1, 4))[0] == want_eval
        assert hyrax.check(key, row_coms, m(point), proof, m([c])[0]) is True
        bad = list(proof)
        bad[3] = proof[3].copy()
        bad[3][0, 0] ^= np.uint64(1)
        assert hyrax.check(key, row_coms, m(point), tuple(bad), m([c])[0]) is False
    finally:
        key.close()
