"""InnerProductArgPC::setup / trim over ed_on_bls12_381 on the device: the kernel bodies of csrc/te_setup.hpp as compiled for gfx950
(the case tables of tests/harness/tesetupprobe.py, bit for bit against the Python restatement AND word for word against the host
build), pc_hip_te_sample_generators and pc_hip_te_srs_prefix against tests/harness/te_setup.py on the Montgomery bytes, and
te_ipa.setup / trim end to end: a key made on the device, a commitment, an opening equal to the harness's on the reference's key, and
the check.  Every launch is a few hundred lanes."""
import ctypes as C

import numpy as np
import pytest

from harness import te_ipa as H
from harness import te_setup as S
from harness import teref as E
from harness import tesetupprobe as P

pytestmark = pytest.mark.gpu
CURVE = "ed_on_bls12_381"
NAME = S.PROTOCOL_NAME
INVALID_ARG, RESIDENT_BYTES = -1, 96


# ---- the probe tables on the device --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    import poly_commit_amd as pc
    pc.load_library()          # brings torch's bundled HIP runtime up first, whichever test file runs first
    return P.T.device_probe()


@pytest.fixture(scope="module")
def host():
    return P.T.host_probe()


def test_probe_sqrt(dev, host):
    assert P.check_sqrt(dev, host) == 4 + 33 * 3


def test_probe_digest(dev, host):
    assert P.check_digest(dev, host) == 3 * (5 + 5 * 3)


def test_probe_from_random_bytes(dev, host):
    assert P.check_try(dev, host) == 14 + sum(S.generator(NAME, i)[1] for i in range(16))


def test_probe_sample_body(dev, host):
    assert P.check_sample(dev, host) == 64 + 1 + 2


# ---- pc_hip_te_sample_generators -----------------------------------------------------------------------------------------------------

def sample(ctx, name, first, count):
    """-> (points, digest counts) of a generated key, read back and freed"""
    key, digests = ctx.te_sample_generators(CURVE, name, first, count, want_digests=True)
    try:
        assert len(key) == count
        return [E.point_from_bytes(row.tobytes()) for row in key.read(0, count)], [int(x) for x in digests]
    finally:
        key.free()


@pytest.mark.parametrize("first,count", [(0, 1), (0, 63), (0, 64), (0, 65), (0, 257), (1000, 16), ((1 << 32) - 2, 4)])
def test_sample_generators_bit_exact(ctx, first, count):
    """the wave, block and normalisation-tile edges; the 16-digest index 1008; an index crossing the 32-bit word of le64"""
    assert sample(ctx, NAME, first, count) == S.generators(NAME, first, count)


def test_sample_generators_without_digest_counts(ctx):
    key = ctx.te_sample_generators(CURVE, NAME, 0, 5)
    try:
        assert [E.point_from_bytes(row.tobytes()) for row in key.read(0, 5)] == S.generators(NAME, 0, 5)[0]
    finally:
        key.free()


def test_slices_agree(ctx):
    a, c = 37, 100
    pts, counts = sample(ctx, NAME, 0, a + c)
    assert sample(ctx, NAME, a, c) == (pts[a:], counts[a:])


@pytest.mark.parametrize("name", P.NAMES, ids=lambda n: "%d bytes" % len(n))
def test_name_lengths(ctx, name):
    """0, 10 and 48 bytes; with 48 the retry message is exactly one 64-byte block"""
    pts, counts = sample(ctx, name, 0, 32)
    assert (pts, counts) == S.generators(name, 0, 32)
    assert max(counts) > 1, "none of the 32 indices retried"


def raw_sample(ctx, curve, name, name_len, first, count):
    h = C.c_void_p()
    rc = ctx.lib.pc_hip_te_sample_generators(ctx.h, curve, name, name_len, first, count, None, C.byref(h))
    assert h.value is None or rc == 0
    return rc, h


def test_argument_errors(ctx):
    ctx.te_sample_generators(CURVE, NAME, 0, 8).free()                              # the context's grow-only workspace is there before the count
    before = ctx.bytes_resident()
    assert raw_sample(ctx, 0, bytes(49), 49, 0, 4)[0] == INVALID_ARG               # the name is too long
    assert raw_sample(ctx, 0, NAME, len(NAME), 0, 0)[0] == INVALID_ARG             # no generators
    assert raw_sample(ctx, 0, NAME, len(NAME), (1 << 64) - 3, 4)[0] == INVALID_ARG  # first_index + count leaves 64 bits
    for curve in (1, 2, -1):
        assert raw_sample(ctx, curve, NAME, len(NAME), 0, 4)[0] == INVALID_ARG
    rc, h = raw_sample(ctx, 0, NAME, len(NAME), (1 << 64) - 5, 4)                   # the last four indices that fit
    assert rc == 0
    ctx.lib.pc_hip_te_srs_free(h)
    key = ctx.te_sample_generators(CURVE, NAME, 0, 8)
    try:
        for count in (0, 9):
            out = C.c_void_p()
            assert ctx.lib.pc_hip_te_srs_prefix(ctx.h, key.h, count, C.byref(out)) == INVALID_ARG and out.value is None
    finally:
        key.free()
    after = ctx.bytes_resident()
    assert (after["device_total"], after["n_keys"]) == (before["device_total"], before["n_keys"])      # no refused call left a key behind


# ---- pc_hip_te_srs_prefix ------------------------------------------------------------------------------------------------------------

def test_prefix(ctx):
    n = 100
    key = ctx.te_sample_generators(CURVE, NAME, 0, n)
    try:
        whole = key.read(0, n)
        assert [E.point_from_bytes(row.tobytes()) for row in whole] == S.generators(NAME, 0, n)[0]
        assert key.bytes_resident()["bases"] == n * RESIDENT_BYTES
        for count in (1, 64, n):
            # a twisted Edwards key is counted in the context's device total and in its number of keys (pc_hip.h)
            before = ctx.bytes_resident()
            pre = key.prefix(count)
            try:
                made = ctx.bytes_resident()
                assert made["device_total"] == before["device_total"] + count * RESIDENT_BYTES and made["n_keys"] == before["n_keys"] + 1
                assert len(pre) == count and (pre.read(0, count) == whole[:count]).all()
                assert pre.bytes_resident()["bases"] == count * RESIDENT_BYTES and pre.fold_table_info() == 0
                assert pre.in_subgroup() is True
                held = ctx.bytes_resident()["device_total"]
            finally:
                pre.free()
            after = ctx.bytes_resident()
            assert after["device_total"] == held - count * RESIDENT_BYTES and after["n_keys"] == before["n_keys"]
        assert (key.read(0, n) == whole).all() and len(key) == n                # the source is unchanged
        assert key.in_subgroup() is True
        # independent of what the library knows by construction: the same points uploaded are asked through the ladder
        up = ctx.upload_te_srs(CURVE, whole)
        try:
            assert up.in_subgroup() is True
        finally:
            up.free()
    finally:
        key.free()


# ---- setup, trim, commit, open, check ------------------------------------------------------------------------------------------------

def rand_scalars(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


def mont(v):
    return E.scalars_array([v], True)[0]


def test_setup_trim_commit_open_check(ctx):
    import torch
    from poly_commit_amd import te_ipa as D
    pp = D.setup(ctx, 200)
    ck = None
    try:
        gens = S.generators(NAME, 0, 258)[0]                                 # 255 + 3: the key, then s, then h
        assert pp["max_degree"] == 255 and len(pp["comm_key"]) == 256
        assert E.point_from_bytes(pp["h"].tobytes()) == gens[257] and E.point_from_bytes(pp["s"].tobytes()) == gens[256]
        with pytest.raises(ValueError, match="TrimmingDegreeTooLarge"):
            D.trim(pp, 256)
        ck = D.trim(pp, 100)
        n = 128
        assert len(ck["comm_key"]) == n and ck["supported_degree"] == n - 1 and len(pp["comm_key"]) == 256
        # the harness's opening on the reference's key
        key, h_point = gens[:n], gens[257]
        coeffs = rand_scalars(4100, n)
        z, xi = rand_scalars(4200, 2)
        comm = E.msm(key, coeffs)
        want_proof, want_rc = H.open(key, h_point, coeffs, comm, z, xi)
        value = H.dot(coeffs, H.powers(z, n))
        # the device's, on the key it made
        cdev = torch.from_numpy(E.scalars_array(coeffs, True)).cuda()
        got_comm, _ = ck["comm_key"].msm(cdev, n=n, montgomery=True)
        assert E.point_from_bytes(got_comm.tobytes()) == comm
        (l, r, fk, c), rc = D.ipa_open(ctx, ck["comm_key"], ck["h"], cdev, got_comm, mont(z), mont(xi))
        pts = lambda arr: [E.point_from_bytes(row.tobytes()) for row in arr]      # noqa: E731
        assert D.fr_to_int(rc) == want_rc
        assert (pts(l), pts(r), E.point_from_bytes(fk.tobytes()), H.fr_int(c)) == want_proof
        assert D.ipa_check(ctx, ck["comm_key"], ck["h"], got_comm, mont(z), mont(value), (l, r, fk, c), mont(xi))
        bad = np.array(c, copy=True)
        bad[0] ^= 1
        assert not D.ipa_check(ctx, ck["comm_key"], ck["h"], got_comm, mont(z), mont(value), (l, r, fk, bad), mont(xi))
    finally:
        if ck is not None:
            ck["comm_key"].free()
        pp["comm_key"].free()
