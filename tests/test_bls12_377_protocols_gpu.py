"""BLS12-377 on the protocol paths above the kernels: the Brakedown code on its 253-bit Fr, streaming_kzg on a true SRS of 4097
powers, and the group entry points with two contexts on device 0 -- every comparison bit for bit.

Checkers: tests/harness/brakedown.py on the fourth field (its modulus and digests from the private copy of the Python reference,
tests/harness/ref377.py), tests/harness/skzg.py (generic over the modulus) with the trapdoor -- a proof over scalars s is
(sum s[d] tau^d) G, one mul_g --, and the copy itself."""
import numpy as np
import pytest

from harness import brakedown as BD
from harness import ipa377 as I
from harness import ref377 as B
from harness import skzg as S

pytestmark = pytest.mark.gpu
R, CURVE, FR, r = B.R, B.CURVE, B.FR, B.RMOD
T = 1024                       # the fold / division tile in coefficients (csrc/skzg.hpp)
N_SRS = 4097


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def _scalars(seed, n):
    return R.gen_scalars(FR, seed, n)


def _mont(vals):
    return B.fr_mont(vals) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def _point(exponent):
    """exponent * G as the library's words (all zero = infinity)"""
    return B.point(B.mul_g(exponent) if exponent % r else None)


# ---- 5. Brakedown on the 253-bit Fr --------------------------------------------------------------------------------------------------

def _messages(code, rows, seed):
    """random rows; from two rows on, a row of all r - 1 and a row of all 0 among them (the encoder's accumulation form is chosen by
    the field's spare top bits)"""
    msgs = BD.messages(code, rows, seed)
    if rows >= 2:
        msgs[0], msgs[rows - 1] = [r - 1] * code.m, [0] * code.m
    return msgs


def _check_encode(ctx, code, row_counts, seed):
    import torch
    dev_code = code.upload(ctx)
    try:
        assert dev_code.codeword_len == code.m_ext and code.p == r
        for rows in row_counts:
            msgs = _messages(code, rows, seed + rows)
            want = [BD.encode(code, m) for m in msgs]
            flat = np.ascontiguousarray(BD.monts(CURVE, [x for row in msgs for x in row]).reshape(rows, code.m, 4))
            raw = dev_code.encode(flat)
            assert [BD.ints(CURVE, raw[i]) for i in range(rows)] == want, (code.m, rows, "host -> host")
            assert all(v < r for v in B.ints(raw.reshape(-1, 4))), "canonical residues"
            y = I.filled((rows, code.m_ext, 4))
            dev_code.encode(_dev(flat), rows=rows, out=y)
            torch.cuda.synchronize()
            assert (y.cpu().numpy().view(np.uint64) == raw).all(), (code.m, rows, "device -> device")
    finally:
        dev_code.free()


@pytest.mark.parametrize("nv", [10, 12])
def test_brakedown_encode_default_codes(ctx, nv):
    n, code = BD.default_code(CURVE, nv, 0x3771000 + nv)
    _check_encode(ctx, code, sorted({1, 2, n}), 0x77)


def test_brakedown_encode_ragged_and_base_codes(ctx):
    _check_encode(ctx, BD.ragged_code(CURVE), (1, 2, 3, 65), 0x88)
    _check_encode(ctx, BD.base_code(CURVE, 17), (1, 2, 64), 0x99)


def test_brakedown_commit_equals_restatement_and_the_three_steps(ctx):
    nv, col_hash, tree_hash, len_prefix = 12, "blake2s", "sha256", True
    n, code = BD.default_code(CURVE, nv, 0x3772000)
    evals = BD.messages(BD.base_code(CURVE, 1 << nv), 1, 0x21)[0]
    evals[:code.m] = [r - 1] * code.m                                     # the first row of the matrix: all r - 1
    evals[code.m:2 * code.m] = [0] * code.m
    want = BD.ref_commit(code, n, evals, col_hash, tree_hash, len_prefix)
    dev_code = code.upload(ctx)
    try:
        mat = np.ascontiguousarray(BD.monts(CURVE, evals).reshape(n, code.m, 4))
        ext = np.zeros((n, code.m_ext, 4), dtype=np.uint64)
        nodes, leaves = dev_code.commit(mat, col_hash=col_hash, tree_hash=tree_hash, len_prefix=len_prefix, ext_out=ext)
        assert [BD.ints(CURVE, ext[i]) for i in range(n)] == want["ext"]
        assert [bytes(x) for x in leaves] == want["leaves"]
        assert [bytes(x) for x in nodes] == want["nodes"] and bytes(nodes[0]) == want["root"]
        ext2 = dev_code.encode(mat)
        leaves2 = ctx.column_hash(CURVE, ext2, col_hash)
        nodes2 = ctx.merkle_tree(leaves2, tree_hash, len_prefix)
        assert (ext2 == ext).all() and (leaves2 == leaves).all() and (nodes2 == nodes).all()
    finally:
        dev_code.free()


def test_multilinear_brakedown_commit_open_check(ctx):
    nv = 12
    n, code = BD.default_code(CURVE, nv, 0x3773000 + nv)
    evals, point = _scalars(0x31, 1 << nv), _scalars(0x32, nv)
    evals[code.m:2 * code.m] = [r - 1] * code.m
    want = BD.ref_commit(code, n, evals)
    dev_code = code.upload(ctx)
    try:
        com, state = BD.commit(ctx, code, dev_code, n, _dev(BD.monts(CURVE, evals)))
        assert (com["n_rows"], com["n_cols"], com["n_ext_cols"], com["root"]) == (n, code.m, code.m_ext, want["root"])
        t = BD.num_queries(CURVE, code.m_ext)
        assert t == R.calculate_t(253, 128, (61 * 1000, 1521 * 1000), code.m_ext) and 0 < t <= code.m_ext
        idx = [(i * 7919 + 13) % code.m_ext for i in range(t)]
        idx[0], idx[1] = code.m_ext - 1, code.m_ext - 2
        ab = BD.tensor(CURVE, point, code.m)
        rr = _scalars(0x33, n)
        pr = BD.open(ctx, code, state, idx, BD.monts(CURVE, rr), ab)
        want_pr = BD.ref_open(code, want, idx, rr, ab)
        assert BD.ints(CURVE, pr["v"]) == want_pr["v"] and BD.ints(CURVE, pr["well_formedness"]) == want_pr["well_formedness"]
        assert [BD.ints(CURVE, c) for c in pr["columns"]] == want_pr["columns"] and pr["paths"] == want_pr["paths"]
        value = R.mle_evaluate(FR, evals, point)
        assert sum(x * y for x, y in zip(want_pr["v"], ab[0])) % r == value
        args = (ctx, code, dev_code, com)
        rm = BD.monts(CURVE, rr)
        assert BD.check(*args, BD.monts(CURVE, [value])[0], pr, idx, rm, ab) is True
        assert BD.ref_check(code, want, value, want_pr, idx, rr, ab) is True
        assert BD.check(*args, BD.monts(CURVE, [value + 1])[0], pr, idx, rm, ab) is False
        bad = dict(pr); bad["columns"] = pr["columns"].copy(); bad["columns"][1, 0, 0] ^= np.uint64(1)
        with pytest.raises(BD.InvalidCommitment):
            BD.check(*args, BD.monts(CURVE, [value])[0], bad, idx, rm, ab)
        bad = dict(pr); bad["paths"] = list(pr["paths"])
        i0, sib, path = bad["paths"][2]
        bad["paths"][2] = (i0, sib, [bytes([path[0][0] ^ 1]) + path[0][1:]] + list(path[1:]))
        with pytest.raises(BD.InvalidCommitment):
            BD.check(*args, BD.monts(CURVE, [value])[0], bad, idx, rm, ab)
        bad = dict(pr); bad["well_formedness"] = pr["well_formedness"].copy(); bad["well_formedness"][0, 0] ^= np.uint64(1)
        with pytest.raises(BD.InvalidCommitment):
            BD.check(*args, BD.monts(CURVE, [value])[0], bad, idx, rm, ab)
    finally:
        dev_code.free()


# ---- 5b. column digests chained over row slabs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hash_name", ["blake2s", "sha256"])
def test_column_digests_chained_over_row_slabs(ctx, hash_name):
    """pc_hip_column_hash_part on the 253-bit Fr: the chaining state of every column handed from slab to slab (even slabs, an odd last
    slab, one slab that is first and last, two column ranges per slab) gives the copy's column digests, as pc_hip_column_hash over the
    whole matrix does; an odd slab that is not the last is refused.  A row of all r - 1 and a row of all 0 among the rows."""
    import torch
    import poly_commit_amd as pc
    rows, n_cols = 23, 96
    can = _scalars(0x51AB, rows * n_cols)
    can[n_cols:2 * n_cols], can[7 * n_cols:8 * n_cols] = [r - 1] * n_cols, [0] * n_cols
    mat = B.fr_mont(can).reshape(rows, n_cols, 4)
    want = np.stack([np.frombuffer(R.column_digest(FR, [can[i * n_cols + j] for i in range(rows)], hash_name), dtype=np.uint8) for j in range(n_cols)])
    assert (ctx.column_hash(CURVE, mat, hash_name) == want).all()
    dev = _dev(mat)
    for cuts in ([0, 23], [0, 8, 23], [0, 2, 4, 22, 23], [0, 10, 20, 23]):
        state = torch.zeros((n_cols, 12), dtype=torch.int32, device="cuda")
        out = torch.zeros((n_cols, 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for k in range(len(cuts) - 1):
            lo, hi = cuts[k], cuts[k + 1]
            for c0, c1 in ((0, 40), (40, n_cols)):
                ctx.column_hash_part(CURVE, dev.data_ptr() + lo * n_cols * 32, hi - lo, n_cols, rows, state.data_ptr(), k == 0, k == len(cuts) - 2,
                                     out.data_ptr(), hash_name, c0, c1 - c0)
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint8).reshape(n_cols, 32) == want).all(), cuts
    state = torch.zeros((n_cols, 12), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(pc.PcHipError):
        ctx.column_hash_part(CURVE, dev.data_ptr(), 3, n_cols, rows, state.data_ptr(), True, False, 0, hash_name)


# ---- 6. streaming_kzg on a true SRS ----------------------------------------------------------------------------------------------------

TAU = _scalars(0xBE7A377, 1)[0]


@pytest.fixture(scope="module")
def true_srs(ctx):
    """tau^i G, i <= 4096, made by pc_hip_fixed_base_batch_mul from the powers of a known tau (as tests/test_bls12_377_gpu.py does)"""
    import torch
    powers = S.powers(TAU, N_SRS, r)
    out = torch.empty((N_SRS, 12), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(CURVE, B.point(B.G), _dev(B.fr_mont(powers)).data_ptr(), N_SRS, out.data_ptr())
    srs = ctx.upload_srs(CURVE, out.data_ptr(), n=N_SRS)
    for i in (0, 1, 2048, N_SRS - 1):
        assert (srs.read(i, 1)[0] == _point(powers[i])).all(), i
    yield srs
    srs.free()


def _lg(n):
    return max(1, (n - 1).bit_length())


def _points(k):
    """k points: 0 among them (k >= 2), one repeated (k >= 3)"""
    pts = _scalars(0x9017 + k, k)
    if k >= 2:
        pts[1] = 0
    if k >= 3:
        pts[2] = pts[0]
    return pts


@pytest.mark.parametrize("n", [1, 5, T - 1, T, T + 1, 2 * T + 1])
def test_fold_tree_every_level(ctx, n):
    f = _scalars(0xF01D + n, n)
    fm = _mont(f)
    for depth in sorted({1, _lg(n), _lg(n) + 2}):
        rhos = _scalars(0xF01E + depth, depth)
        want = S.fold_tree(f, rhos, r)
        total = sum(len(lv) for lv in want)
        for src in (fm, _dev(fm)):
            out = I.filled((total + 1, 4))
            offs = ctx.fold_tree(CURVE, src if isinstance(src, np.ndarray) else src.data_ptr(), _mont(rhos), out.data_ptr(), total, n=n)
            assert offs == [sum(len(lv) for lv in want[:i]) for i in range(depth)]
            got = out.cpu().numpy().view(np.uint64)
            assert (got[total] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the last level"
            assert B.fr_from_mont(got[:total]) == [c for lv in want for c in lv], (n, depth)
        with pytest.raises(Exception):
            ctx.fold_tree(CURVE, fm, _mont(rhos), out.data_ptr(), total - 1, n=n)      # capacity below sum L_i


@pytest.mark.parametrize("k", [1, 3, 16])
def test_poly_div_multi(ctx, k):
    """lengths around k, the groups (64), the tile, and past it the division scan's fan-in boundaries (8 x 16 = 128, 8 x 256 = 2048)"""
    for pts in ([_points(k)] if k > 1 else [_points(1), [0]]):
        zs = _mont(pts)
        for n in sorted({k, k + 1, 64, 65, T, T + 1, T + 128, 2048 + k, 4097}):
            f = _scalars(0xD17 + n, n)
            if n > 3:
                f[-1] = 0
            want_q, want_r = S.div_multi(f, pts, r)
            q, rem = ctx.poly_div_multi(CURVE, _mont(f), zs)
            assert B.fr_from_mont(q) == want_q and B.fr_from_mont(rem) == want_r, (n, k)
            _, rem2 = ctx.poly_div_multi(CURVE, _dev(_mont(f)).data_ptr(), zs, n=n, want_quotient=False)
            assert (rem2 == rem).all(), (n, k)


@pytest.mark.parametrize("n", [3, T + 1, 4097])
def test_kzg_open_multi(ctx, true_srs, n):
    f = _scalars(0x09E4 + n, n)
    pts = _points(3)
    proof, inf, rem = true_srs.kzg_open_multi(_mont(f), _mont(pts))
    want_rem, want_e = S.open_multi(f, pts, TAU, r)
    assert (want_rem, want_e) == S.space_open_multi_points(S.reversed_key(TAU, N_SRS, r), list(reversed(f)), pts, r)
    assert B.fr_from_mont(rem) == want_rem and (proof == _point(want_e)).all() and inf == (want_e == 0), n
    # one point: the single-point opening and the evaluation
    z = pts[:1]
    proof1, inf1, rem1 = true_srs.kzg_open_multi(_dev(_mont(f)).data_ptr(), _mont(z), n=n)
    single, sinf = true_srs.kzg_open(_mont(f), _mont(z)[0])
    want_q = R.witness_polynomial(FR, f, z[0])
    assert (proof1 == single).all() and inf1 == sinf and (proof1 == _point(S.msm_exponent(want_q, TAU, r))).all()
    assert B.fr_from_mont(rem1) == [R.poly_eval(FR, f, z[0])]


def test_kzg_batch_open_multi(ctx, true_srs):
    """a ragged batch at 5 points (0 and a repeat among them) with a 128-bit eta, host and device input; a batch with no polynomial
    longer than k: the identity"""
    pts = _points(5)
    eta = _scalars(0xE7A, 1)[0] >> 125
    lens = [101, 7, 1, 300, 5, 64, T + 1]
    polys = [_scalars(0xBA7C + j, ln) for j, ln in enumerate(lens)]
    want = _point(S.batch_open_multi(polys, pts, eta, TAU, r))
    proof, inf = true_srs.kzg_batch_open_multi([_mont(f) for f in polys], _mont(pts), _mont([eta])[0])
    assert (proof == want).all() and not inf
    devs = [_dev(_mont(f)) for f in polys]
    proof_d, _ = true_srs.kzg_batch_open_multi([d.data_ptr() for d in devs], _mont(pts), _mont([eta])[0], lens=lens)
    assert (proof_d == want).all()
    short = [_scalars(5, 4), _scalars(6, 5)]
    proof, inf = true_srs.kzg_batch_open_multi([_mont(f) for f in short], _mont(pts), _mont([eta])[0])
    assert inf and not proof.any()


def _check_commit_folding(srs, f, depth):
    rhos = _scalars(0xC0F0 + depth, depth)
    want = S.commit_folding(f, rhos, TAU, r)
    assert want == S.space_commit_folding(S.reversed_key(TAU, N_SRS, r), list(reversed(f)), rhos, r)
    got, inf = srs.kzg_commit_folding(_mont(f), _mont(rhos))
    for i in range(depth):
        assert (got[i] == _point(want[i])).all() and bool(inf[i]) == (want[i] == 0), (len(f), depth, i)
    dev, dinf = srs.kzg_commit_folding(_dev(_mont(f)).data_ptr(), _mont(rhos), n=len(f))
    assert (dev == got).all() and (dinf == inf).all()
    return got, want


@pytest.mark.parametrize("n", [5, T + 1, 4097])
def test_kzg_commit_folding(ctx, true_srs, n):
    f = _scalars(0xC0FF + n, n)
    f[-1] = 0                                                           # a zero leading coefficient
    _check_commit_folding(true_srs, f, _lg(n))
    if n == 5:
        _check_commit_folding(true_srs, f, _lg(n) + 2)
        # f[2b] = -rho_0 f[2b + 1]: level 1 (and every level below it) is all zero
        rho0 = _scalars(0xC0F0 + 3, 3)[0]
        odd = _scalars(0x0DD, 4)
        g = [c for o in odd for c in ((-rho0 * o) % r, o)]
        got, want = _check_commit_folding(true_srs, g, 3)
        assert want == [0, 0, 0] and not got.any()


@pytest.mark.parametrize("n", [5, T + 1, 4097])
def test_kzg_open_folding(ctx, true_srs, n):
    depth = _lg(n)
    f = _scalars(0x0F01 + n, n)
    rhos, etas, pts = _scalars(0x0F02, depth), _scalars(0x0F03, depth), _points(3)
    want_rem, want_e = S.open_folding(f, rhos, pts, etas, TAU, r)
    assert (want_rem, want_e) == S.space_open_folding(S.reversed_key(TAU, N_SRS, r), list(reversed(f)), rhos, pts, etas, r)
    before = true_srs.read(0, N_SRS).copy()
    args = (_mont(f), _mont(rhos), _mont(pts), _mont(etas))
    rem, proof, inf = true_srs.kzg_open_folding(*args)
    assert [B.fr_from_mont(rem[i]) for i in range(depth)] == want_rem, n
    assert (proof == _point(want_e)).all() and inf == (want_e == 0), n
    rem2, proof2, inf2 = true_srs.kzg_open_folding(*args)               # again on the same key: identical
    assert (rem2 == rem).all() and (proof2 == proof).all() and inf2 == inf
    assert (true_srs.read(0, N_SRS) == before).all()


# ---- 7. the group entry points, two contexts on device 0 --------------------------------------------------------------------------------

def test_group_two_contexts_batch_async_ntt_ligero(ctx, true_srs):
    """pc_hip_group_msm_batch, _commit_open_async + _job_wait, _ntt_batch and _ligero_commit: each the single-context result, which is
    itself compared with the copy in this test"""
    import poly_commit_amd as pc
    _, words = B.gen_bases(N_SRS)
    g = pc.Group([0, 0])
    try:
        # MSM batch on P_i = (i + 1) G: a whole key, a short prefix, a prefix that ends one past the middle
        lens = [N_SRS, 300, 2050]
        polys = [_scalars(0x377900 + j, m) for j, m in enumerate(lens)]
        host = [B.fr_mont(q) for q in polys]
        one = ctx.upload_srs(CURVE, words)
        single = one.msm_batch(host, lens, host=True)
        one.free()
        for table in (False, True):
            gs = g.upload_srs(CURVE, words, precompute=table)
            got = gs.msm_batch(host)
            gs.free()
            for j, q in enumerate(polys):
                assert (got[j] == single[j]).all() and (got[j] == B.point(B.closed_form(q))).all(), (table, j)
        # commit + open, asynchronously, on the true SRS
        powers = true_srs.read(0, N_SRS)
        gs = g.upload_srs(CURVE, powers)
        coeffs, z = _scalars(0x377910, N_SRS), _scalars(0x377911, 1)[0]
        mont, zm = B.fr_mont(coeffs), B.fr_mont([z])[0]
        jobs = [gs.commit_open_async(mont, zm), gs.commit_open_async(mont[:1000], zm)]
        for job, m in zip(jobs, (N_SRS, 1000)):
            comm, proof, val = job.wait()
            f = coeffs[:m]
            assert (comm == true_srs.msm(mont[:m], montgomery=True)[0]).all() and (comm == _point(R.poly_eval(FR, f, TAU))).all(), m
            assert (proof == true_srs.kzg_open(mont[:m], zm)[0]).all(), m
            assert (proof == _point(R.poly_eval(FR, R.witness_polynomial(FR, f, z), TAU))).all(), m
            assert (val == ctx.poly_eval(CURVE, mont[:m], zm)).all() and B.fr_from_mont(val) == [R.poly_eval(FR, f, z)], m
        gs.free()
        # NTT: 3 rows of 2^11
        co = [_scalars(0x377920 + j, 1 << 11) for j in range(3)]
        mat = np.stack([B.fr_mont(c) for c in co])
        got = g.ntt_batch(CURVE, mat, 11)
        assert (got == ctx.ntt_batch(CURVE, mat, 11)).all()
        assert [B.fr_from_mont(got[j]) for j in range(3)] == [R.ntt(FR, c, 11) for c in co]
        # Ligero commit of 4096 coefficients
        coeffs = _scalars(0x377930, 4096)
        st = R.ligero_commit(FR, coeffs)
        n_rows, n_cols = st["n_rows"], st["n_cols"]
        mat = B.fr_mont(coeffs + [0] * (n_rows * n_cols - len(coeffs))).reshape(n_rows, n_cols, 4)
        log_n = st["n_ext_cols"].bit_length() - 1
        nodes, leaves = g.ligero_commit(CURVE, mat, log_n)
        nodes1, leaves1 = ctx.ligero_commit(CURVE, mat, log_n)
        assert (nodes == nodes1).all() and (leaves == leaves1).all()
        assert nodes.tobytes() == b"".join(st["nodes"]) and [leaves[j].tobytes() for j in range(1 << log_n)] == st["leaves"]
        assert nodes[0].tobytes() == st["root"]
    finally:
        g.close()
