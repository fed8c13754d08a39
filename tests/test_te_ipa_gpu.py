"""The device path of InnerProductArgPC over ed_on_bls12_381 against the pure-Python restatements tests/harness/teref.py and
tests/harness/te_ipa.py, bit-exact on the Montgomery bytes: the vector kernels of the rounds over the 252-bit scalar field, the
out-of-place key fold with and without the key's fold table (operands of low order and outside the prime-order subgroup included:
expected values are integer-exact), the subgroup check, the rounds as one call under every route (table / ladder first fold, folding /
fixed key late rounds), and the driver poly_commit_amd/te_ipa.py."""
import numpy as np
import pytest

from harness import te_ipa as H
from harness import teref as E

pytestmark = pytest.mark.gpu
CURVE = "ed_on_bls12_381"
NPTS = 8192
NKEY = 1024


def key_scalars(n):
    return [(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % E.R for i in range(n)]


@pytest.fixture(scope="module")
def pts():
    """8192 known multiples of G"""
    return E.fixed_base(E.GEN).mul_many(key_scalars(NPTS))


def rand_scalars(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


def dev(ks):
    import torch
    return torch.from_numpy(E.scalars_array(ks, True)).cuda()


def ints(t):
    ri = pow(E.MONT_R, -1, E.R)
    out = []
    for row in t.cpu().numpy():
        v = int.from_bytes(row.tobytes(), "little")
        assert v < E.R, "a scalar left [0, r)"
        out.append(v * ri % E.R)
    return out


def mont(v):
    return E.scalars_array([v], True)[0]


def points_of(arr):
    return [E.point_from_bytes(row.tobytes()) for row in arr]


U_DENSE = int("55" * 31, 16) % E.R            # 0101..01: no two adjacent ones, every second NAF position non-zero
U_SET = [0, 1, 2, E.R - 1, E.R - 2, U_DENSE, 1 << 251, rand_scalars(7, 1)[0]]


# ---- Fr kernels ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_te_fr_powers(ctx, n):
    import torch
    for z in (0, 1, E.R - 1, rand_scalars(n, 1)[0]):
        out = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")
        ctx.te_fr_powers(CURVE, mont(z), n, out)
        assert ints(out[:n]) == H.powers(z, n), z
        assert not out[n].any()                                                  # nothing behind the n-th power


@pytest.mark.parametrize("m", [1, 2, 4, 512, 1024, 1 << 13])
def test_te_ipa_fold_dots(ctx, m):
    """with and without the fold at size 2m; 1024 is the first size with more than one workgroup"""
    rnd = rand_scalars(m, 4 * m)
    u = rand_scalars(m + 1, 1)[0]
    ui = pow(u, -1, E.R)
    vectors = {"r-1": ([E.R - 1] * (2 * m), [E.R - 1] * (2 * m)),
               "0/1": ([i & 1 for i in range(2 * m)], [(i >> 1) & 1 for i in range(2 * m)]),
               "random": (rnd[:2 * m], rnd[2 * m:])}
    for name, (c, z) in vectors.items():
        dc, dz = dev(c), dev(z)
        got = ctx.te_ipa_fold_dots(CURVE, dc, dz, m)
        assert (H.fr_int(got[0]), H.fr_int(got[1])) == H.fold_dots(list(c), list(z), m), name
        assert ints(dc) == c and ints(dz) == z, name                             # no fold: the vectors are only read
        wc, wz = list(c), list(z)
        want = H.fold_dots(wc, wz, m, u, ui)
        got = ctx.te_ipa_fold_dots(CURVE, dc, dz, m, mont(u), mont(ui))
        assert (H.fr_int(got[0]), H.fr_int(got[1])) == want, name
        assert ints(dc) == wc and ints(dz) == wz, name                           # folded below m, untouched from m on


def test_te_ipa_key_scalars(ctx):
    """n0 = 64: the rounds at m = 64 .. 2 with the fold of the round before applied first, then the final fold of size 2"""
    import torch
    n0 = 64
    c = rand_scalars(1, n0)
    dc, s = dev(c), dev([1] * n0)
    s_want = [1] * n0
    us = rand_scalars(2, 8)
    m, k, u_prev = n0, 0, None
    while m >= 2:
        out = torch.zeros((2 * n0, 32), dtype=torch.uint8, device="cuda")
        if u_prev is not None:
            s_want = H.key_scalars_fold(s_want, 2 * m, u_prev)
        ctx.te_ipa_key_scalars(CURVE, dc, m, s, n0, fold_u=None if u_prev is None else mont(u_prev), fold_m=2 * m if u_prev is not None else 0,
                               out_l_dev=out[:n0], out_r_dev=out[n0:])
        want_l, want_r = H.key_scalars_lr(c, s_want, m)
        assert ints(s) == s_want and ints(out[:n0]) == want_l and ints(out[n0:]) == want_r, m
        u_prev, k, m = us[k], k + 1, m // 2
    ctx.te_ipa_key_scalars(CURVE, None, 0, s, n0, fold_u=mont(u_prev), fold_m=2)
    assert ints(s) == H.key_scalars_fold(s_want, 2, u_prev)


# ---- the out-of-place fold and the fold table -------------------------------------------------------------------------------------------

def special_key(pts, n_half, u):
    """2 n_half points and the expected fold by u: known multiples of G (expected values by the fixed-base table) with the special
    entries in the upper half -- the points of order 2, 4 and 8, P + T8, an all-zero entry -- and a lane whose result is the identity"""
    key = list(pts[:2 * n_half])
    kk = key_scalars(2 * n_half)
    special = {0: E.T2, 1: E.T4, 2: E.T8, 3: E.add(key[n_half + 3], E.T8) if n_half > 3 else None, 4: E.ZERO}
    special = {i: p for i, p in special.items() if i < n_half and p is not None}
    for i, p in special.items():
        key[n_half + i] = p
    if n_half > 5:
        key[5] = E.neg(E.mul(u, key[n_half + 5]))
        special[5] = None
    want = E.fixed_base(E.GEN).mul_many([(kk[i] + u * kk[n_half + i]) % E.R for i in range(n_half)])
    for i in special:
        want[i] = E.add(key[i], E.mul(u, key[n_half + i]))
    if n_half > 5:
        assert want[5] == E.IDENT
    return key, want


@pytest.mark.parametrize("n_half", [1, 15, 16, 17, 255, 257, 1024])
def test_te_ec_fold_from(ctx, pts, n_half):
    us = U_SET if n_half <= 64 else [E.R - 2, U_SET[-1]]
    for u in us:
        key, want = special_key(pts, n_half, u)
        arr = E.points_array(key)
        k = ctx.upload_te_srs(CURVE, arr)
        try:
            plain = k.ec_fold_from(n_half, mont(u))                               # no table: the ladder
            assert k.fold_table_info() == 0
            k.precompute_fold()
            assert k.fold_table_info() == 253
            tabled = k.ec_fold_from(n_half, mont(u))
            try:
                assert len(plain) == n_half and len(tabled) == n_half
                got = plain.read(0, n_half)
                assert points_of(got) == want, u
                assert (tabled.read(0, n_half) == got).all(), u                   # the same points, bit for bit
                assert (k.read(0, 2 * n_half) == arr).all()                       # src is untouched
                # an MSM over the folded key reads its rebuilt third coordinate
                m = max(1, n_half // 2)
                ks = rand_scalars(n_half, m)
                out, _ = tabled.msm(E.scalars_array(ks, False), n=m)
                assert E.point_from_bytes(out.tobytes()) == E.msm(want[:m], ks), u
            finally:
                plain.free()
                tabled.free()
        finally:
            k.free()


@pytest.mark.parametrize("n_half", [4095, 4096])
def test_te_ec_fold_from_table_against_the_in_place_fold(ctx, pts, n_half):
    """several workgroups: the table fold against pc_hip_te_ec_fold (pinned to Python by test_te_gpu.py) on an uploaded copy"""
    arr = E.points_array(pts[:2 * n_half])
    u = mont(rand_scalars(n_half, 1)[0])
    k, copy = ctx.upload_te_srs(CURVE, arr).precompute_fold(), ctx.upload_te_srs(CURVE, arr)
    try:
        out = k.ec_fold_from(n_half, u)
        copy.ec_fold(n_half, u)
        try:
            assert (out.read(0, n_half) == copy.read(0, n_half)).all()
            assert (k.read(0, 2 * n_half) == arr).all()
        finally:
            out.free()
    finally:
        k.free()
        copy.free()


def test_te_fold_table_other_half_and_in_place_fold(ctx, pts):
    """a key with a table folded at another n_half runs the ladder; the in-place fold drops the table it makes stale"""
    arr = E.points_array(pts[:64])
    u = rand_scalars(64, 1)[0]
    k = ctx.upload_te_srs(CURVE, arr).precompute_fold()
    try:
        out = k.ec_fold_from(16, mont(u))
        try:
            assert points_of(out.read(0, 16)) == E.fold(pts[:32], u)
        finally:
            out.free()
        k.ec_fold(32, mont(u))
        assert k.fold_table_info() == 0 and k.bytes_resident()["fold_table"] == 0
        assert points_of(k.read(0, 32)) == E.fold(pts[:64], u)
    finally:
        k.free()


def test_te_fold_table_residency_and_argument_checks(pts):
    import poly_commit_amd as pc
    from poly_commit_amd import PcHipError
    c, other = pc.Context(0), pc.Context(0)
    try:
        n = 100
        k = c.upload_te_srs(CURVE, E.points_array(pts[:n]))
        before = c.bytes_resident()
        assert k.bytes_resident()["fold_table"] == 0
        k.precompute_fold()
        assert k.bytes_resident()["fold_table"] == 253 * (n // 2) * 96
        assert c.bytes_resident()["fold_tables"] == before["fold_tables"] + 253 * (n // 2) * 96
        k.free()
        assert c.bytes_resident()["fold_tables"] == before["fold_tables"]
        k = c.upload_te_srs(CURVE, E.points_array(pts[:n]))
        odd = c.upload_te_srs(CURVE, E.points_array(pts[:33]))
        u = mont(3)
        with pytest.raises(PcHipError):
            odd.precompute_fold()                                                 # n must be even
        with pytest.raises(PcHipError):
            k.ec_fold_from(n // 2 + 1, u)                                         # 2 n_half > len
        with pytest.raises(PcHipError):
            k.ec_fold_from(0, u)
        lib = c.lib
        import ctypes as C
        h = C.c_void_p()
        up = C.c_void_p(u.ctypes.data)
        assert lib.pc_hip_te_ec_fold_from(other.h, k.h, 4, up, C.byref(h)) == -1   # a foreign context
        assert lib.pc_hip_te_srs_precompute_fold(other.h, k.h) == -1
        flag = C.c_int(0)
        assert lib.pc_hip_te_srs_in_subgroup(other.h, k.h, C.byref(flag)) == -1
        assert lib.pc_hip_te_ec_fold_from(c.h, k.h, 4, None, C.byref(h)) == -1 and lib.pc_hip_te_ec_fold_from(c.h, k.h, 4, up, None) == -1
        assert lib.pc_hip_te_srs_in_subgroup(c.h, k.h, None) == -1 and lib.pc_hip_te_srs_fold_table_info(k.h, None) == -1
        assert (k.read(0, n) == E.points_array(pts[:n])).all()
        # a table that was never released goes with the context
        k.precompute_fold()
    finally:
        c.close()
        other.close()
    c2 = pc.Context(0)
    assert c2.bytes_resident()["fold_tables"] == 0
    c2.close()
    k.free()
    odd.free()


# ---- the subgroup check -------------------------------------------------------------------------------------------------------------------

def test_te_srs_in_subgroup(ctx, pts):
    n = 600

    def answer(key):
        k = ctx.upload_te_srs(CURVE, E.points_array(key))
        try:
            first = k.in_subgroup()
            assert k.in_subgroup() == first                                       # the cached answer
            return first
        finally:
            k.free()
    assert answer(pts[:n]) is True
    for i in (0, n - 1, 256):
        key = list(pts[:n])
        key[i] = E.add(key[i], E.T2)
        assert answer(key) is False, i
    assert answer([E.T8]) is False
    key = list(pts[:n])
    key[77] = E.ZERO
    assert answer(key) is True
    assert answer([E.IDENT, E.ZERO]) is True


# ---- the rounds as one call -----------------------------------------------------------------------------------------------------------------

H_POINT = E.mul(0x1234567, E.GEN)
_ref = {}


def reference(pts, n, key=None, tag=""):
    """the harness's opening of a polynomial of n coefficients on key[:n], computed once per size and shared"""
    if (n, tag) not in _ref:
        key = list(pts[:n]) if key is None else key
        coeffs = rand_scalars(1000 + n, n)
        z, xi = rand_scalars(2000 + n, 2)
        comm = E.msm(key, coeffs)
        proof, rc = H.open(key, H_POINT, coeffs, comm, z, xi)
        _ref[(n, tag)] = dict(coeffs=coeffs, z=z, xi=xi, comm=comm, proof=proof, rc=rc, value=H.dot(coeffs, H.powers(z, n)))
    return _ref[(n, tag)]


def device_open(k, ref, n, fixed_key_below):
    """pc_hip_te_ipa_open_rounds on the combined polynomial, with the harness's transcript: (l_vec, r_vec, final_comm_key, c) as points / an integer"""
    state = {"rc": ref["rc"]}

    def next_challenge(l, r):
        state["rc"] = H.challenge(H.ser_fr(state["rc"]) + H.ser_point(E.point_from_bytes(l.tobytes())) + H.ser_point(E.point_from_bytes(r.tobytes())))
        return H.fr_bytes(state["rc"])
    comb = dev([ref["xi"] * v % E.R for v in ref["coeffs"]])
    h_prime = E.points_array([E.mul(ref["rc"], H_POINT)])[0]
    l, r, fk, c = k.ipa_open_rounds(comb, n, mont(ref["z"]), h_prime, next_challenge, fixed_key_below)
    return points_of(l), points_of(r), E.point_from_bytes(fk.tobytes()), H.fr_int(c)


@pytest.fixture(scope="module")
def keys(ctx, pts):
    arr = E.points_array(pts[:NKEY])
    plain, tabled = ctx.upload_te_srs(CURVE, arr), ctx.upload_te_srs(CURVE, arr).precompute_fold()
    yield plain, tabled, arr
    plain.free()
    tabled.free()


@pytest.mark.parametrize("n", [1, 2, 8, 1 << 9, 1 << 10])
def test_te_ipa_open_rounds_every_route(ctx, pts, keys, n):
    plain, tabled, arr = keys
    ref = reference(pts, n)
    for k in (plain, tabled):
        for fkb in (1, 64, n, 0):
            assert device_open(k, ref, n, fkb) == ref["proof"], (n, fkb, k is tabled)
    # two openings in a row gave equal proofs (each equals the harness's) and the committer keys are as they were
    assert (plain.read(0, NKEY) == arr).all() and (tabled.read(0, NKEY) == arr).all()
    assert tabled.fold_table_info() == 253 and plain.in_subgroup()
    if n == NKEY:
        assert H.check(list(pts[:n]), H_POINT, ref["comm"], ref["z"], ref["value"], ref["proof"], ref["xi"])


def test_te_ipa_open_rounds_folds_on_a_key_outside_the_subgroup(ctx, pts):
    """P + T8 among the points and fixed_key_below = 64: per-base factors modulo r would be wrong, the library folds in every round
    and stays integer-exact"""
    n = 128
    key = list(pts[:n])
    key[5] = E.add(key[5], E.T8)
    key[100] = E.add(key[100], E.T8)
    ref = reference(pts, n, key, "t8")
    k = ctx.upload_te_srs(CURVE, E.points_array(key))
    try:
        assert device_open(k, ref, n, 64) == ref["proof"]
        assert k.in_subgroup() is False
        assert device_open(k, ref, n, 0) == ref["proof"]
    finally:
        k.free()


def test_te_ipa_driver_open_and_check(ctx, pts):
    from poly_commit_amd import te_ipa as D
    n = 512
    ref = reference(pts, n)
    k = ctx.upload_te_srs(CURVE, E.points_array(pts[:n])).precompute_fold()
    try:
        coeffs = dev(ref["coeffs"])
        h_xy, comm = E.points_array([H_POINT])[0], E.points_array([ref["comm"]])[0]
        got_comm, _ = k.msm(coeffs, n=n, montgomery=True)
        assert (got_comm == comm).all()
        (l, r, fk, c), rc = D.ipa_open(ctx, k, h_xy, coeffs, comm, mont(ref["z"]), mont(ref["xi"]))
        assert D.fr_to_int(rc) == ref["rc"]
        assert (points_of(l), points_of(r), E.point_from_bytes(fk.tobytes()), H.fr_int(c)) == ref["proof"]
        assert ints(coeffs) == ref["coeffs"]                                      # the caller's polynomial is left as it is
        assert D.ipa_check(ctx, k, h_xy, comm, mont(ref["z"]), mont(ref["value"]), (l, r, fk, c), mont(ref["xi"]))
        assert not D.ipa_check(ctx, k, h_xy, comm, mont(ref["z"]), mont(ref["value"] + 1), (l, r, fk, c), mont(ref["xi"]))
        assert H.check(list(pts[:n]), H_POINT, ref["comm"], ref["z"], ref["value"], ref["proof"], ref["xi"])
    finally:
        k.free()
