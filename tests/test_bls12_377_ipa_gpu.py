"""BLS12-377 on the IPA entry points: the Fr kernels of the halving rounds against Python integers, the key fold (GLV ladder, fold
tables) at the challenges and lanes where a split or a recoding can go wrong, the opening loop and one whole proof -- every word
that a call returns compared bit for bit.

The C++ oracle does not know the curve.  The checker is the private copy of the Python reference (tests/harness/ref377.py) and,
for everything that holds thousands of points, discrete logarithms (tests/harness/ipa377.py): keys are d_i G with known d_i, made
on the device by pc_hip_fixed_base_batch_mul and checked at their ends, two interior points and every infinity."""
import numpy as np
import pytest

from harness import ipa377 as I
from harness import ref377 as B

pytestmark = pytest.mark.gpu
R, CURVE, FR, r = B.R, B.CURVE, B.FR, B.RMOD
LAM = I.glv_constants()["lam"]
LENGTHS = (1, 2, 255, 256, 257, 4097)


def _m(v):
    return B.fr_mont([v])[0]


def _rand(seed):
    return R.gen_scalars(FR, seed, 1)[0]


def _edgy(seed, n):
    """random elements with 0, 1 and r - 1 among them"""
    v = R.gen_scalars(FR, seed, n)
    for i, e in zip((0, n // 2, n - 1), (0, 1, r - 1)):
        v[i] = e
    return v


def _read(t):
    return B.fr_from_mont(t.cpu().numpy().view(np.uint64))


# ---- 1. the Fr kernels of the rounds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
def test_fr_powers(ctx, n):
    for z in (0, 1, r - 1, _rand(0x5001 + n)):
        out = I.filled((n + 1, 4))
        ctx.fr_powers(CURVE, _m(z), n, out.data_ptr())
        want = [1] * n
        for i in range(1, n):
            want[i] = want[i - 1] * z % r
        got = out.cpu().numpy().view(np.uint64)
        assert B.ints(got[:n]) == B.ints(B.fr_mont(want)), (n, hex(z))
        assert (got[n] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the end"


@pytest.mark.parametrize("n", LENGTHS)
def test_fr_dot_and_fr_fold(ctx, n):
    a, b, top = _edgy(0x5100 + n, n), _edgy(0x5200 + n, n), [r - 1] * n
    dev = {k: I.dev(B.fr_mont(v)) for k, v in (("a", a), ("b", b), ("top", top))}
    vals = {"a": a, "b": b, "top": top}
    for x, y in (("a", "b"), ("a", "top"), ("top", "top")):               # all r - 1: the largest sum a reduction sees
        got = ctx.fr_dot(CURVE, dev[x].data_ptr(), dev[y].data_ptr(), n)
        assert B.ints(got.reshape(1, 4)) == B.ints(B.fr_mont([sum(p * q for p, q in zip(vals[x], vals[y]))])), (n, x, y)
    for s in (0, 1, r - 1, _rand(0x5300 + n)):
        for x, y in (("a", "b"), ("top", "top"), ("a", "top")):
            lo, hi = I.copy_of(dev[x]), I.copy_of(dev[y])
            ctx.fr_fold(CURVE, lo.data_ptr(), hi.data_ptr(), n, _m(s))
            assert _read(lo) == [(p + s * q) % r for p, q in zip(vals[x], vals[y])], (n, hex(s), x, y)
            assert (hi == dev[y]).all()


@pytest.mark.parametrize("m", [2, 4, 256, 512, 1024, 8192])
def test_ipa_fold_dots(ctx, m):
    """one lane, one block, several blocks with the k_ipa_dots_final pass: the two inner products without a fold, and with the fold
    at size 2m by (u, u^-1) -- the folded coefficients and powers element for element, the upper halves left alone"""
    q = m // 2
    dots = lambda c, z: [sum(x * y for x, y in zip(c[q:m], z[:q])) % r, sum(x * y for x, y in zip(c[:q], z[q:m])) % r]      # noqa: E731
    for cs, zs in ((_edgy(0x5400 + m, 2 * m), _edgy(0x5500 + m, 2 * m)), ([r - 1] * (2 * m), [r - 1] * (2 * m))):
        c, z = I.dev(B.fr_mont(cs[:m])), I.dev(B.fr_mont(zs[:m]))
        got = ctx.ipa_fold_dots(CURVE, c.data_ptr(), z.data_ptr(), m)
        assert B.fr_from_mont(got) == dots(cs, zs), m
        assert _read(c) == cs[:m] and _read(z) == zs[:m]
        for u in (1, r - 1, _rand(0x5600 + m)):
            ui = pow(u, -1, r)
            c, z = I.dev(B.fr_mont(cs)), I.dev(B.fr_mont(zs))
            got = ctx.ipa_fold_dots(CURVE, c.data_ptr(), z.data_ptr(), m, _m(u), _m(ui))
            fc = [(cs[i] + ui * cs[m + i]) % r for i in range(m)]
            fz = [(zs[i] + u * zs[m + i]) % r for i in range(m)]
            assert _read(c) == fc + cs[m:] and _read(z) == fz + zs[m:], (m, hex(u))
            assert B.fr_from_mont(got) == dots(fc, fz), (m, hex(u))


@pytest.mark.parametrize("n0", [4, 64, 4096])
def test_ipa_key_scalars(ctx, n0):
    """The fixed-key rounds as poly_commit_amd/ipa.py drives them: s = (1, ..), then per round the pending fold of s by the previous
    challenge at size 2m and the round's two scalar vectors at size m, and the last fold of size 2.  Checked against the definition:
    s_j *= u where (j mod fold_m) >= fold_m / 2;  out_l[j] = c[h + i] s_j for i = j mod m < h = m / 2, else 0;  out_r[j] = c[i - h] s_j
    for i >= h, else 0 -- and that definition against the rounds themselves: with the key d_j G, sum_j out_l[j] d_j is the logarithm
    ipa_rounds_dlog gives for L (h' = 0), and sum_j s_j d_j the one of the final key."""
    import torch
    d = R.gen_scalars(FR, 0x5700 + n0, n0)
    coeffs = _edgy(0x5800 + n0, n0)
    lg = n0.bit_length() - 1
    ch = [1, r - 1][:max(0, lg - 1)] + R.gen_scalars(FR, 0x5900 + n0, lg)
    ch = ch[:lg]
    want_l, want_r, want_key, _ = I.ipa_rounds_dlog(d, 0, coeffs, 1, ch)
    s_dev = torch.empty((n0, 4), dtype=torch.int64, device="cuda")
    ctx.fr_powers(CURVE, _m(1), n0, s_dev.data_ptr())
    s, cs, m, u_prev = [1] * n0, list(coeffs), n0, None
    for k in range(lg):
        h = m // 2
        c_dev = I.dev(B.fr_mont(cs[:m]))
        out = I.filled((2 * n0 + 1, 4))
        ctx.ipa_key_scalars(CURVE, c_dev.data_ptr(), m, s_dev.data_ptr(), n0, fold_u=None if u_prev is None else _m(u_prev),
                            fold_m=0 if u_prev is None else 2 * m, out_l_dev=out.data_ptr(), out_r_dev=out.data_ptr() + 32 * n0)
        if u_prev is not None:
            s = [x * u_prev % r if (j & (2 * m - 1)) >= m else x for j, x in enumerate(s)]
        ol = [cs[h + (j & (m - 1))] * s[j] % r if (j & (m - 1)) < h else 0 for j in range(n0)]
        orr = [cs[(j & (m - 1)) - h] * s[j] % r if (j & (m - 1)) >= h else 0 for j in range(n0)]
        got = out.cpu().numpy().view(np.uint64)
        assert _read(s_dev) == s, (n0, k)
        assert B.fr_from_mont(got[:n0]) == ol and B.fr_from_mont(got[n0:2 * n0]) == orr, (n0, k)
        assert (got[2 * n0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the end"
        assert sum(x * y for x, y in zip(ol, d)) % r == want_l[k] and sum(x * y for x, y in zip(orr, d)) % r == want_r[k]
        ui = pow(ch[k], -1, r)
        cs = [(cs[i] + ui * cs[h + i]) % r for i in range(h)]
        u_prev, m = ch[k], h
    ctx.ipa_key_scalars(CURVE, None, 0, s_dev.data_ptr(), n0, fold_u=_m(u_prev), fold_m=2)          # the last fold (size 2)
    s = [x * u_prev % r if j & 1 else x for j, x in enumerate(s)]
    assert _read(s_dev) == s
    assert sum(x * y for x, y in zip(s, d)) % r == want_key
    # the fold alone, without scalar vectors, at a size in the middle (ipa_check's use)
    if n0 >= 64:
        u = _rand(0x5A00)
        ctx.ipa_key_scalars(CURVE, None, 0, s_dev.data_ptr(), n0, fold_u=_m(u), fold_m=16)
        assert _read(s_dev) == [x * u % r if (j & 15) >= 8 else x for j, x in enumerate(s)]


# ---- 2. the key fold on a table-free key ---------------------------------------------------------------------------------------------

LONGEST_SPLIT_BITS = 127        # what the seeded search of ipa377.longest_split finds (tests/test_bls12_377_cpu.py finds it on the CPU)
CHALLENGES = I.edge_challenges()
SPECIALS = {3: "kl_inf", 17: "kr_inf", 30: "both_inf", 41: "doubling", 64: "cancel"}      # lane 64 opens the second wave


def _fold_both_ways(ctx, half, u, seed, **kw):
    """pc_hip_ec_fold_from (a new key, the source untouched) and pc_hip_ec_fold (in place, the upper half untouched) on the key of
    fold_case: every point of both results"""
    d, want, _, _ = I.fold_case(half, u, seed, **kw)
    key = I.device_key(ctx, d)
    want = B.points(want)
    srs = ctx.upload_srs(CURVE, key)
    try:
        out = srs.fold_from(half, _m(u))
        got = out.read(0, half)
        out.free()
        assert (got == want).all(), ("fold_from", half, hex(u), np.nonzero((got != want).any(axis=1))[0][:8])
        assert (srs.read(0, 2 * half) == key).all()
        srs.ec_fold(half, _m(u))
        got = srs.read(0, half)
        assert (got == want).all(), ("ec_fold", half, hex(u), np.nonzero((got != want).any(axis=1))[0][:8])
        assert (srs.read(half, half) == key[half:]).all()
    finally:
        srs.free()
    return want


@pytest.mark.parametrize("name,u", CHALLENGES, ids=[c[0] for c in CHALLENGES])
def test_ec_fold_edge_challenges_and_special_lanes(ctx, name, u):
    """half = 65: every challenge with K_l, K_r or both at infinity, u K_r = K_l (the closing addition doubles) and u K_r = -K_l (the
    result is the all-zero infinity) beside ordinary lanes of the same wave"""
    if name == "longest split":
        assert max(abs(k) for k in I.glv_split(u)).bit_length() == LONGEST_SPLIT_BITS
    want = _fold_both_ways(ctx, 65, u, 0x6000 + len(name), specials=SPECIALS)
    assert not want[64].any() and (u == 0 or want[41].any())


@pytest.mark.parametrize("half", [1, 63, 64, 65, 4095, 4096])
def test_ec_fold_sizes(ctx, half):
    """the 64-lane launch edge and the switch at half >= 4096 to Jacobian results normalised in batches (JacBatchAffineBody): the random
    challenge and lambda, an infinity in each half"""
    kw = dict(inf_lo=half // 3, inf_hi=half // 2) if half > 1 else {}
    for name, u in CHALLENGES:
        if name in ("random", "lambda") or (half < 4095 and name in ("r-1", "longest split")):
            _fold_both_ways(ctx, half, u, 0x6100 + half, **kw)


def _other_curve_case(curve, u_int, half):
    """the same lanes for a curve the C++ oracle knows: (key, expected fold), the oracle's u K_r[i] + K_l[i]"""
    import oracle_lib as O
    from poly_commit_amd.ipa import _neg_point
    cid = O.CURVES[curve]
    pool = np.ascontiguousarray(O.gen_bases(curve, 2 * half))
    lo, hi = pool[:half].copy(), pool[half:].copy()
    u = O.ints_to_limbs([u_int], 4)

    def mul(P):
        out = np.zeros_like(P)
        O.lib().orc_ec_mul(cid, O.p64(np.ascontiguousarray(P)), O.p64(u[0]), O.p64(out))
        return out
    for i, kind in SPECIALS.items():
        if kind in ("kl_inf", "both_inf"):
            lo[i] = 0
        if kind in ("kr_inf", "both_inf"):
            hi[i] = 0
        if kind == "doubling":
            lo[i] = mul(hi[i])
        if kind == "cancel":
            lo[i] = _neg_point(curve, mul(hi[i]))
    want = np.zeros_like(lo)
    for i in range(half):
        O.lib().orc_ec_add(cid, O.p64(mul(hi[i])), O.p64(np.ascontiguousarray(lo[i])), O.p64(want[i]))
    return np.ascontiguousarray(np.concatenate([lo, hi])), want, O.fr_mont_array(curve, [u_int])[0]


@pytest.mark.parametrize("curve", ["bls12_381", "pallas"])
def test_ec_fold_edge_challenges_on_the_oracle_curves(ctx, curve):
    """the edge-challenge list (each curve's own lambda and longest split) and the special lanes at half = 65 on BLS12-381 and Pallas,
    against the C++ oracle: no curve had the fold tested away from one random challenge"""
    import pyref
    p = pyref.FIELDS[pyref.CURVES[curve]["fr"]]["p"]
    for name, u in I.edge_challenges(p, curve):
        key, want, um = _other_curve_case(curve, u, 65)
        assert not want[64].any() and not want[30].any()
        srs = ctx.upload_srs(curve, key)
        try:
            out = srs.fold_from(65, um)
            got = out.read(0, 65)
            out.free()
            assert (got == want).all(), (curve, name, "fold_from")
            assert (srs.read(0, 130) == key).all()
            srs.ec_fold(65, um)
            assert (srs.read(0, 65) == want).all(), (curve, name, "ec_fold")
            assert (srs.read(65, 65) == key[65:]).all()
        finally:
            srs.free()


# ---- 3. fold tables ------------------------------------------------------------------------------------------------------------------

N_TABLE = 1 << 10
U_SETS = {"random": (_rand(0x7001), _rand(0x7002)), "lambda, r-1": (LAM, r - 1), "1, lambda": (1, LAM), "r-1, 1": (r - 1, 1)}


@pytest.fixture(scope="module")
def table_keys(ctx):
    """per (u1, u2): a key of 2^10 points with an infinity in each half whose fold by u1 is a chain, its expected fold and double
    fold (logarithms: the chain again, e_i + u2 e_(q + i)), and both as the table-free ladder computes them"""
    h, q = N_TABLE // 2, N_TABLE // 4
    out = {}
    for name, (u1, u2) in U_SETS.items():
        d, want1, e, delta = I.fold_case(h, u1, 0x7100 + len(name), inf_lo=5, inf_hi=h // 2 + 7)
        words = I.device_key(ctx, d)
        e2 = [(e[i] + u2 * e[q + i]) % r for i in range(q)]
        want2 = I.points_of_logs(e2, delta * (1 + u2) % r)
        plain = ctx.upload_srs(CURVE, words)
        k1 = plain.fold_from(h, _m(u1))
        ladder1 = k1.read(0, h).copy()
        k1.ec_fold(q, _m(u2))
        ladder2 = k1.read(0, q).copy()
        k1.free()
        plain.free()
        out[name] = dict(d=d, words=words, want1=B.points(want1), want2=B.points(want2), ladder1=ladder1, ladder2=ladder2)
    return out


def test_fold_ladder_equals_the_logarithms(table_keys):
    for name, t in table_keys.items():
        assert (t["ladder1"] == t["want1"]).all() and (t["ladder2"] == t["want2"]).all(), name


@pytest.mark.parametrize("form", [None, (1, 3), (2, 2), (2, 3), (2, 4)], ids=["library's choice", "1 level w3", "2 levels w2", "2 levels w3", "2 levels w4"])
def test_fold_tables(ctx, table_keys, form):
    """pc_hip_srs_precompute_fold[_ex] on a resident key: fold_from(n / 2) and fold2_from(n / 4) out of every form of the table equal
    the ladder and the logarithms; round 2's commitments by linearity (pc_hip_ipa_round2_msms); the committer key stays as it is"""
    n, h, q = N_TABLE, N_TABLE // 2, N_TABLE // 4
    for name, (u1, u2) in U_SETS.items():
        t = table_keys[name]
        srs = ctx.upload_srs(CURVE, t["words"])
        try:
            if form is None:
                srs.precompute_fold()
                # the library's choice: below 2^16 points no second level (that fold is a latency-bound ladder either way), and the
                # widest digits it takes unasked, 4 -- 25 MB here, far inside its share of the device's free memory
                levels, w = srs.fold_table_info()
                assert (levels, w) == (1, 4)
            else:
                srs.precompute_fold(*form)
                assert srs.fold_table_info() == form
                levels, w = form
            assert srs.bytes_resident()["fold_table"] == (131 << (w - 2)) * (n - (n >> levels)) * 96
            k1 = srs.fold_from(h, _m(u1))
            got1 = k1.read(0, h)
            k1.free()
            assert (srs.read(0, n) == t["words"]).all()
            assert (got1 == t["ladder1"]).all() and (got1 == t["want1"]).all(), (name, form)
            k2 = srs.fold2_from(q, _m(u1), _m(u2))
            got2 = k2.read(0, q)
            k2.free()
            assert (srs.read(0, n) == t["words"]).all()
            assert (got2 == t["ladder2"]).all() and (got2 == t["want2"]).all(), (name, form)
            if name == "random":
                cs = R.gen_scalars(FR, 0x7200, 2 * q)
                c_dev = I.dev(B.fr_mont(cs))
                l, r_ = srs.ipa_round2_msms(c_dev.data_ptr(), q, _m(u1))
                d = t["d"]
                want_l = sum(cs[q + i] * (d[i] + u1 * d[2 * q + i]) for i in range(q))
                want_r = sum(cs[i] * (d[q + i] + u1 * d[3 * q + i]) for i in range(q))
                assert (l == B.point(B.mul_g(want_l))).all() and (r_ == B.point(B.mul_g(want_r))).all(), form
                assert (srs.read(0, n) == t["words"]).all() and srs.fold_table_info() == (levels, w)
        finally:
            srs.free()


# ---- 4. the opening loop ---------------------------------------------------------------------------------------------------------------

def _opening_key(ctx, n, seed):
    d = R.gen_scalars(FR, seed, n + 1)
    for i in ((5, n // 2 + 7) if n >= 16 else (1, n // 2 + 1)):                # an infinity in each half
        d[i] = 0
    words = I.device_key(ctx, d)
    return d[:n], np.ascontiguousarray(words[:n]), d[n], words[n]


def _open_and_check(ctx, key, d, h_log, h_words, n, fkb, python_loop, seed):
    from poly_commit_amd import ipa
    lg = n.bit_length() - 1
    coeffs, point, ch = R.gen_scalars(FR, seed, n), _rand(seed + 1), R.gen_scalars(FR, seed + 2, lg)
    coeffs[n // 2 - 1] = 0
    l_logs, r_logs, key_log, c = I.ipa_rounds_dlog(d, h_log, coeffs, point, ch)
    want = I.log_points(l_logs + r_logs + [key_log])
    it = iter(B.fr_mont(ch))
    tm = {}
    l, r_, fk, got_c = ipa.ipa_open_rounds(ctx, CURVE, key, I.dev(B.fr_mont(coeffs)), n, _m(point), h_words, lambda L, R_: next(it), timings=tm,
                                          fixed_key_below=fkb, python_loop=python_loop)
    assert (l == want[:lg]).all() and (r_ == want[lg:2 * lg]).all(), (n, fkb, python_loop)
    assert (fk == want[2 * lg]).all() and B.fr_from_mont(got_c) == [c], (n, fkb, python_loop)
    return tm


@pytest.mark.parametrize("n,fkb", [(4, None), (1 << 8, 16), (1 << 10, 0), (1 << 10, None), (1 << 13, 64)])
def test_ipa_open_rounds(ctx, n, fkb):
    """pc_hip_ipa_open_rounds and the same sequence driven round by round, on a key handed over as a host array: key folded in every
    round (0), never (None: the fixed key from the start), and the switch in the middle"""
    d, words, h_log, h_words = _opening_key(ctx, n, 0x8000 + n)
    for python_loop in (False, True):
        _open_and_check(ctx, words, d, h_log, h_words, n, fkb, python_loop, 0x8100 + n)


@pytest.mark.parametrize("tables", ["one level", "two levels", "none"])
@pytest.mark.parametrize("n,fkb", [(4, None), (1 << 8, 16), (1 << 10, 0), (1 << 10, None), (1 << 13, 64)])
def test_ipa_open_rounds_on_a_resident_key(ctx, n, fkb, tables):
    """two openings in a row on the same resident key -- with its window table and a one-level fold table (1, 3), with its window table
    and a two-level table (2, 3), with no table -- each through both loops; the committer key reads back untouched.  Every size takes
    every table: n = 4 accepts both forms (the two-level one covers K[1 .. 4)) and, below 8 points, opens without the deferred first
    round; (2^10, 0) with two levels is the deferred round, the double fold out of the table, then ladder folds down to one point."""
    from poly_commit_amd import ipa
    d, words, h_log, h_words = _opening_key(ctx, n, 0x8200 + n)
    srs = ctx.upload_srs(CURVE, words)
    try:
        if tables != "none":
            form = (1, 3) if tables == "one level" else (2, 3)
            srs.precompute(min_pairs=1)
            srs.precompute_fold(*form)
            assert srs.fold_table_info() == form
        for rep in range(2):
            for python_loop in (False, True):
                tm = _open_and_check(ctx, srs, d, h_log, h_words, n, fkb, python_loop, 0x8300 + n + 16 * rep)
                kinds = tm.get("ec_fold_kind", [])
                limit = fkb if fkb is not None else (ipa.FIXED_KEY_BELOW if python_loop else ipa.library_fixed_key_below())
                if tables == "two levels" and n >= 8 and n // 2 > limit:
                    assert kinds[:2] == ["deferred", "table2"], kinds
                    if fkb == 0:
                        assert kinds[2:] == ["ladder"] * (n.bit_length() - 3), kinds
                elif tables == "one level" and n > limit:
                    assert kinds[0] == "table1", kinds
            assert (srs.read(0, n) == words).all()
    finally:
        srs.free()


def test_ipa_whole_proof_with_the_transcript(ctx):
    """InnerProductArgPC::open of two polynomials at n = 32 (combination, Blake2s transcript over ark-serialize bytes, rounds) against
    the copy's ipa_open on real points; ipa_check accepts the proof and refuses it with one wrong value"""
    from poly_commit_amd import ipa
    n = 32
    pts, words = B.gen_bases(n + 1)
    key, key_words, h = list(pts[:n]), words[:n].copy(), pts[n]
    key[3], key_words[3] = None, 0
    d = [0 if i == 3 else i + 1 for i in range(n)]
    polys = [R.gen_scalars(FR, 0x9000 + j, n - 3 * j) for j in range(2)]
    comms = [B.mul_g(sum(c * x for c, x in zip(q, d))) for q in polys]
    xi, point = R.gen_scalars(FR, 0x9010, 2), _rand(0x9011)
    wl, wr, wfk, wc, _ = R.ipa_open(CURVE, key, h, polys, comms, point, xi)
    comm_words = [B.point(A) for A in comms]
    srs = ctx.upload_srs(CURVE, key_words)
    try:
        for k in (key_words, srs):
            dev = [I.dev(B.fr_mont(q)) for q in polys]
            (l, r_, fk, c), _ = ipa.ipa_open(ctx, CURVE, k, words[n], [t.data_ptr() for t in dev], [len(q) for q in polys], comm_words, _m(point), B.fr_mont(xi))
            assert (l == B.points(wl)).all() and (r_ == B.points(wr)).all() and (fk == B.point(wfk)).all() and B.fr_from_mont(c) == [wc]
        assert (srs.read(0, n) == key_words).all()
    finally:
        srs.free()
    values = [_m(R.poly_eval(FR, q, point)) for q in polys]
    args = (ctx, CURVE, key_words, words[n], comm_words, _m(point))
    assert ipa.ipa_check(*args, values, (l, r_, fk, c), B.fr_mont(xi)) is True
    bad_c = c.copy(); bad_c[0] ^= np.uint64(1)
    assert ipa.ipa_check(*args, values, (l, r_, fk, bad_c), B.fr_mont(xi)) is False
    bad_v = [values[0].copy(), values[1]]; bad_v[0][1] ^= np.uint64(4)
    assert ipa.ipa_check(*args, bad_v, (l, r_, fk, c), B.fr_mont(xi)) is False
    assert ipa.ipa_check(*args, values, (l, r_, key_words[1], c), B.fr_mont(xi)) is False
