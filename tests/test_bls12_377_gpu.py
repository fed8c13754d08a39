"""BLS12-377 through the C ABI on the device: G1 MSM, KZG commit / open on a true SRS, serialization, the Fr kernels (NTT, column
digests, Ligero commit) and the group entry points -- every comparison bit for bit.

Two checkers that share nothing with the HIP code, and must agree with the device and so with each other: the private copy of the
Python reference (tests/harness/ref377.py) and the C++ oracle (curve id 3; tests/test_oracle_bls12_377_cpu.py holds it against the
copy on its own).  MSM bases are P_i = (i + 1) G wherever possible, so that sum k_i P_i = (sum k_i (i + 1) mod r) G is ONE Python
scalar multiplication; keys with other points carry their discrete logarithms along.  At n <= 64 the copy's naive `msm` is compared
as well.  The larger shapes of the curve run against the oracle in the files of the paths themselves (tests/test_msm_gpu.py, ...)."""
import hashlib

import numpy as np
import pytest

import oracle_lib as O
from harness import ref377 as B

pytestmark = pytest.mark.gpu
R, CURVE, FR, r, p = B.R, B.CURVE, B.FR, B.RMOD, B.P
SIZES = (1, 2, 31, 32, 33, 257, 4097)
NMAX = 4097


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def _want(dlogs, ks):
    """sum k_i (d_i G) as words"""
    return B.point(B.mul_g(sum(k * d for k, d in zip(ks, dlogs))))


@pytest.fixture(scope="module")
def key(ctx):
    """the 4097-point key P_i = (i + 1) G in its three forms: table-free, full window table, GLV window table"""
    pts, words = B.gen_bases(NMAX)
    keys = {"plain": ctx.upload_srs(CURVE, words), "table": ctx.upload_srs(CURVE, words), "glv": ctx.upload_srs(CURVE, words)}
    keys["table"].precompute(min_pairs=1, glv=False)
    keys["glv"].precompute(min_pairs=1, glv=True)
    yield pts, words, keys
    for k in keys.values():
        k.free()


def test_upload_read_and_table_forms(ctx, key):
    pts, words, keys = key
    assert (keys["plain"].read(0, NMAX) == words).all() and (keys["glv"].read(4000, 97) == words[4000:]).all()
    full, half = keys["table"].bytes_resident()["window_tables"], keys["glv"].bytes_resident()["window_tables"]
    assert keys["plain"].bytes_resident()["window_tables"] == 0 and 0 < half <= 0.6 * full, (half, full)


@pytest.mark.parametrize("form", ["plain", "table", "glv"])
def test_msm_parity(ctx, key, form):
    """pc_hip_msm at the direct path, the graph path's lower edge and a multi-chunk sort: host and device scalars, canonical and
    Montgomery form, against the closed form (and the naive sum at n <= 64)"""
    pts, words, keys = key
    srs = keys[form]
    for n in SIZES:
        ks = R.gen_scalars(FR, 0x377000 + n, n)
        want = B.point(B.closed_form(ks))
        if n <= 64:
            assert (want == B.point(R.msm(CURVE, pts[:n], ks))).all()
        canon, mont = B.fr(ks), B.fr_mont(ks)
        assert (O.msm_pippenger(CURVE, words[:n], canon, 8, 1) == want).all() and (O.f_to_mont(CURVE, 1, canon) == mont).all(), n
        dc, dm = _dev(canon), _dev(mont)
        for sc, m in ((canon, False), (mont, True), (dc, False), (dm, True)):
            for rep in range(3 if sc is dc else 1):                                    # a repeated device call is captured, then replayed
                got, inf = srs.msm(sc, n=n, montgomery=m)
                assert (got == want).all() and not inf, (form, n, m, type(sc).__name__, rep)
        if form != "plain":
            assert ctx.last_msm_shape()["window_table"], (form, n)
    # a slice of the key (KZG10::commit skips leading zeros by offsetting the powers), and more scalars than bases left
    ks = R.gen_scalars(FR, 0x377100, 1000)
    got, _ = srs.msm(B.fr(ks), base_offset=1234)
    assert (got == B.point(B.closed_form(ks, first=1235))).all() and (got == O.msm_pippenger(CURVE, np.ascontiguousarray(words[1234:]), B.fr(ks), 8, 1)).all()
    got, _ = srs.msm(B.fr(ks), base_offset=NMAX - 600)
    assert (got == B.point(B.closed_form(ks[:600], first=NMAX - 599))).all()
    job = srs.msm_async(B.fr(ks), base_offset=7)
    got, inf = job.wait()
    assert (got == B.point(B.closed_form(ks, first=8))).all() and not inf


@pytest.mark.parametrize("n", [257, 4097])
def test_msm_edge_sets(ctx, n):
    pts, _ = B.gen_bases(NMAX)
    by_dlog = lambda d: None if d == 0 else (pts[d - 1] if d > 0 else R.ec_neg(CURVE, pts[-d - 1]))
    scalars = B.edge_scalars(n, 0xED6E + n)
    packed = {name: B.fr(ks) for name, ks in scalars.items()}
    for kname, dl in B.edge_keys(n).items():
        words = B.points([by_dlog(d) for d in dl])
        want = {name: _want(dl, ks) for name, ks in scalars.items()}
        for name, sc in packed.items():
            assert (O.msm_pippenger(CURVE, words, sc, 8, 2) == want[name]).all(), (n, kname, name)
        if kname == "P beside -P":                                                      # n is odd: the last point has no partner
            last = B.point(B.mul_g(scalars["equal in pairs"][-1] * dl[-1]))
            assert (want["equal in pairs"] == last).all()
        for form in ("plain", "table", "glv"):
            srs = ctx.upload_srs(CURVE, words)
            if form != "plain":
                srs.precompute(min_pairs=1, glv=form == "glv")
            for name, sc in packed.items():
                got, inf = srs.msm(sc)
                assert (got == want[name]).all() and inf == (not want[name].any()), (n, kname, form, name)
            srs.free()
    # the whole sum cancels: an even number of P, -P pairs with equal scalars
    dl = B.edge_keys(n - 1)["P beside -P"]
    srs = ctx.upload_srs(CURVE, B.points([by_dlog(d) for d in dl]))
    got, inf = srs.msm(B.fr(B.edge_scalars(n - 1, 5)["equal in pairs"]))
    assert inf and not got.any()
    srs.free()


def test_msm_batch_and_many(ctx, key):
    """MarlinKZG10::commit's batch (3 polynomials of 300 coefficients) and Hyrax's rows (5 MSMs of 17 pairs)"""
    pts, words, keys = key
    polys = [R.gen_scalars(FR, 0x377200 + j, 300) for j in range(3)]
    want = [B.point(B.closed_form(q)) for q in polys]
    assert all((O.msm_pippenger(CURVE, words, B.fr(q), 8, 1) == w).all() for q, w in zip(polys, want))
    host = [B.fr_mont(q) for q in polys]
    dev = [_dev(h) for h in host]
    for form, srs in keys.items():
        got = srs.msm_batch([t.data_ptr() for t in dev], [300] * 3)
        assert all((got[j] == want[j]).all() for j in range(3)), form
        got = srs.msm_batch(host, [300] * 3, host=True)
        assert all((got[j] == want[j]).all() for j in range(3)), form
    got = keys["plain"].msm_batch([t.data_ptr() for t in dev], [300, 123, 1], base_offsets=[0, 50, 4096])
    assert (got[0] == want[0]).all() and (got[1] == B.point(B.closed_form(polys[1][:123], first=51))).all()
    assert (got[2] == B.point(B.mul_g(polys[2][0] * 4097))).all()
    rows = [R.gen_scalars(FR, 0x377300 + j, 17) for j in range(5)]
    rows[3] = [0] * 17
    sc = np.stack([B.fr(q) for q in rows])
    for montgomery in (False, True):
        arr = np.stack([B.fr_mont(q) for q in rows]) if montgomery else sc
        got, inf = keys["plain"].msm_many(arr, montgomery=montgomery)
        assert all((got[j] == B.point(B.closed_form(rows[j]))).all() for j in range(5)) and list(inf) == [False, False, False, True, False]
        assert all((got[j] == O.msm_pippenger(CURVE, words, sc[j], 4, 1)).all() for j in range(5))
    got, _ = keys["plain"].msm_many(sc, base_offset=100)
    assert all((got[j] == B.point(B.closed_form(rows[j], first=101))).all() for j in range(5))


def test_host_point_helpers():
    import poly_commit_amd._ffi as F
    pts, words = B.gen_bases(16)
    assert (F.points_sum(CURVE, words[:9]) == B.point(B.mul_g(45))).all()
    both = np.stack([words[3], B.point(R.ec_neg(CURVE, pts[3]))])
    assert not F.points_sum(CURVE, both).any()
    assert (F.points_sum(CURVE, np.stack([words[3], words[3], B.point(None)])) == words[7]).all()
    for k in (0, 1, 2, r - 1, 0x1234567 << 220):
        assert (F.point_mul(CURVE, words[4], B.fr_mont([k])[0]) == B.point(B.mul_g(5 * k))).all(), hex(k)


@pytest.fixture(scope="module")
def true_srs(ctx):
    """beta^i G, i <= 4096, made by pc_hip_fixed_base_batch_mul from the powers of a known beta (KZG10::setup, kzg10/mod.rs:68-76)"""
    import torch
    n = 4097
    beta = R.gen_scalars(FR, 0xBE7A377, 1)[0]
    powers = [1]
    for _ in range(n - 1):
        powers.append(powers[-1] * beta % r)
    pw = _dev(B.fr_mont(powers))
    out = torch.empty((n, 12), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(CURVE, B.point(B.G), pw.data_ptr(), n, out.data_ptr())
    srs = ctx.upload_srs(CURVE, out.data_ptr(), n=n)
    yield beta, srs
    srs.free()


def test_true_srs_points(ctx, true_srs):
    beta, srs = true_srs
    n = srs.n
    for i in (0, 1, n - 1):
        assert (srs.read(i, 1)[0] == B.point(B.mul_g(pow(beta, i, r)))).all(), i
    # the per-lane ladder below 4096 scalars gives the same points as the window-table path above
    import torch
    ks = [0, 1, r - 1, beta]
    out = torch.empty((len(ks), 12), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(CURVE, B.point(B.G), _dev(B.fr_mont(ks)).data_ptr(), len(ks), out.data_ptr())
    got = out.cpu().numpy().view(np.uint64)
    assert all((got[i] == B.point(B.mul_g(k))).all() for i, k in enumerate(ks))


def _open_expected(coeffs, z, beta):
    q = R.witness_polynomial(FR, coeffs, z)
    return q, B.point(B.mul_g(R.poly_eval(FR, q, beta))), R.poly_eval(FR, coeffs, z)


@pytest.mark.parametrize("degree", [31, 4096])
def test_kzg_commit_open(ctx, true_srs, degree):
    """commit = p(beta) G; open = q(beta) G with q = (p - p(z)) / (x - z), value = p(z); the division and evaluation kernels alone"""
    beta, srs = true_srs
    n = degree + 1
    coeffs = R.gen_scalars(FR, 0x377400 + degree, n)
    z = R.gen_scalars(FR, 0x377401, 1)[0]
    mont, zm = B.fr_mont(coeffs), B.fr_mont([z])[0]
    q, want_w, want_v = _open_expected(coeffs, z, beta)
    comm, _ = srs.msm(mont, montgomery=True)
    assert (comm == B.point(B.mul_g(R.poly_eval(FR, coeffs, beta)))).all()
    powers = srs.read(0, n)
    assert (O.kzg_commit(CURVE, powers, mont)[1] == comm).all() and (O.kzg_open(CURVE, powers, mont, zm)[1] == want_w).all()
    assert (O.witness_poly(CURVE, mont, zm) == ctx.witness_poly(CURVE, mont, zm)).all() and B.fr_from_mont(O.poly_eval(CURVE, mont, zm)) == [want_v]
    for src in (mont, _dev(mont)):
        proof, inf = srs.kzg_open(src, zm, n=n)
        assert (proof == want_w).all() and not inf
        assert B.fr_from_mont(ctx.poly_eval(CURVE, src, zm, n=n)) == [want_v]
    assert B.fr_from_mont(ctx.witness_poly(CURVE, mont, zm)) == q
    scan = B.fr_from_mont(ctx.div_scan(CURVE, mont, zm))
    assert scan[1:] == q and scan[0] == want_v
    carry = 0x1234567890abcdef << 100
    scan = B.fr_from_mont(ctx.div_scan(CURVE, mont, zm, carry_in=B.fr_mont([carry])[0]))
    assert scan[0] == (want_v + carry * pow(z, n, r)) % r
    # the verifier's equation with the known trapdoor: C - v G = (beta - z) W
    lhs = R.ec_add(CURVE, B.point_of(comm), R.ec_neg(CURVE, B.mul_g(want_v)))
    assert lhs == R.ec_mul(CURVE, (beta - z) % r, B.point_of(proof))


def test_kzg_leading_zeros_and_lincomb(ctx, true_srs):
    beta, srs = true_srs
    z = R.gen_scalars(FR, 0x377402, 1)[0]
    zm = B.fr_mont([z])[0]
    # 5 leading zero coefficients: KZG10::commit skips them and offsets the powers (kzg10/mod.rs:175-178, :452-461)
    coeffs = [0] * 5 + R.gen_scalars(FR, 0x377403, 295)
    want_c = B.point(B.mul_g(R.poly_eval(FR, coeffs, beta)))
    assert (srs.msm(B.fr_mont(coeffs[5:]), base_offset=5, montgomery=True)[0] == want_c).all()
    assert (srs.msm(B.fr_mont(coeffs), montgomery=True)[0] == want_c).all()
    _, want_w, want_v = _open_expected(coeffs, z, beta)
    assert (srs.kzg_open(B.fr_mont(coeffs), zm)[0] == want_w).all()
    powers = srs.read(0, 300)
    assert (O.kzg_commit(CURVE, powers, B.fr_mont(coeffs))[1] == want_c).all() and (O.kzg_open(CURVE, powers, B.fr_mont(coeffs), zm)[1] == want_w).all()
    assert B.fr_from_mont(ctx.poly_eval(CURVE, B.fr_mont(coeffs), zm)) == [want_v]
    # Marlin's open: p = sum_j xi_j p_j on the device (marlin_pc/mod.rs:281-287), then the opening of p
    import torch
    lens = [4097, 1000, 4096]
    polys = [R.gen_scalars(FR, 0x377410 + j, m) for j, m in enumerate(lens)]
    xi = R.gen_scalars(FR, 0x377420, 3)
    comb = R.fr_lincomb(FR, polys, xi)
    assert B.fr_from_mont(ctx.fr_lincomb(CURVE, [B.fr_mont(q) for q in polys], B.fr_mont(xi))) == comb
    dev = [_dev(B.fr_mont(q)) for q in polys]
    out = torch.empty((4097, 4), dtype=torch.int64, device="cuda")
    ctx.fr_lincomb(CURVE, [d.data_ptr() for d in dev], B.fr_mont(xi), n_out=4097, out=out.data_ptr(), lens=lens)
    assert B.fr_from_mont(out.cpu().numpy().view(np.uint64)) == comb
    _, want_w, want_v = _open_expected(comb, z, beta)
    proof, _ = srs.kzg_open(out.data_ptr(), zm, n=4097)
    assert (proof == want_w).all() and B.fr_from_mont(ctx.poly_eval(CURVE, out.data_ptr(), zm, n=4097)) == [want_v]


def _nine_points():
    pts, _ = B.gen_bases(9)
    larger = lambda A: A if A[1] > p - A[1] else R.ec_neg(CURVE, A)
    out = list(pts)
    out[2] = None                                        # infinity
    out[3] = larger(pts[3])                              # y > -y: YIsNegative, 0x80 in the last byte
    out[4] = R.ec_neg(CURVE, larger(pts[4]))             # y < -y: no flag
    return out


@pytest.mark.parametrize("compressed", [False, True])
def test_serialization(ctx, compressed):
    """ark-ec's generic short-Weierstrass form: 96 / 48 bytes, flags in the top bits of the last byte; decoding a compressed point
    takes a Tonelli-Shanks square root with two-adicity 46"""
    pts = _nine_points()
    words = B.points(pts)
    data = R.ser_g1_vec(CURVE, pts, compressed)
    assert len(data) == 8 + 9 * (48 if compressed else 96)
    srs = ctx.upload_srs(CURVE, words)
    assert srs.serialize(compressed=compressed) == data
    if not compressed:
        assert data[8:] == b"".join(O.ser_point(CURVE, w) for w in words)
    assert srs.serialize(offset=2, count=3, compressed=compressed) == R.ser_g1_vec(CURVE, pts[2:5], compressed)
    srs.free()
    loaded, used = ctx.load_serialized_srs(CURVE, data + b"the fields behind powers_of_g", compressed)
    assert loaded.n == 9 and used == len(data) and (loaded.read(0, 9) == words).all()
    assert loaded.serialize(compressed=compressed) == data
    loaded.free()
    first3, _ = ctx.load_serialized_srs(CURVE, data, compressed, max_points=3)
    assert first3.n == 3 and (first3.read(0, 3) == words[:3]).all()
    first3.free()


def test_serialized_point_off_the_curve_is_refused(ctx):
    import poly_commit_amd as pc
    x = 2
    while pow(x ** 3 + 1, (p - 1) // 2, p) != p - 1:     # x^3 + 1 is not a square: no point has this x
        x += 1
    pts, _ = B.gen_bases(3)
    good = [R.ser_point_compressed(CURVE, A) for A in pts]
    data = (3).to_bytes(8, "little") + good[0] + x.to_bytes(48, "little") + good[2]
    with pytest.raises(pc._ffi.PcHipError) as e:
        ctx.load_serialized_srs(CURVE, data, True)
    assert e.value.status == -1 and "1 serialized point(s) are not on the curve" in str(e.value)
    # uncompressed: a y that does not belong to its x, and a coordinate that is not below the modulus
    bad = bytearray(R.ser_g1_vec(CURVE, pts, False))
    bad[8 + 96 + 48] ^= 1
    bad[8 + 2 * 96:8 + 2 * 96 + 48] = (p + pts[2][0]).to_bytes(48, "little")
    with pytest.raises(pc._ffi.PcHipError) as e:
        ctx.load_serialized_srs(CURVE, bytes(bad), False)
    assert e.value.status == -1 and "2 serialized point(s)" in str(e.value)


def test_universal_params_layout():
    """the curve is a pairing curve: G2 points are 96 / 192 bytes (generic short Weierstrass over Fq2)"""
    import poly_commit_amd._ffi as F
    for compressed, g1, g2 in ((True, 48, 96), (False, 96, 192)):
        data = (2).to_bytes(8, "little") + bytes(2 * g1) + (1).to_bytes(8, "little") + bytes(8 + g1) + bytes(2 * g2) + (1).to_bytes(8, "little") + bytes(8 + g2)
        lay = F.universal_params_layout(CURVE, data, compressed)
        assert lay["n_powers_of_g"] == 2 and lay["n_powers_of_gamma_g"] == 1 and lay["n_neg_powers_of_h"] == 1 and lay["total"] == len(data)
        assert lay["beta_h"] - lay["h"] == g2 and lay["h"] == 8 + 2 * g1 + 8 + 8 + g1


@pytest.mark.parametrize("log_n,in_cols", [(0, 1), (1, 1), (5, 24), (10, 256), (11, 1500), (13, 2048), (16, 40000)])
def test_ntt(ctx, log_n, in_cols):
    """3 rows of in_cols < 2^log_n coefficients against the copy's ntt: the smallest sizes, one tile per pass, tiles of several
    columns, and a size whose zero padding skips stages; the field's two-adicity is 47, so omega_N sits 31 .. 47 squarings below ROOT"""
    rows = 3
    co = [R.gen_scalars(FR, 0x377500 + 16 * log_n + j, in_cols) for j in range(rows)]
    mont = np.stack([B.fr_mont(c) for c in co])
    got = ctx.ntt_batch(CURVE, mont, log_n)
    assert got.shape == (rows, 1 << log_n, 4) and (got == O.ntt_batch(CURVE, mont, log_n)).all()
    for j in range(rows):
        assert B.fr_from_mont(got[j]) == R.ntt(FR, co[j], log_n), (log_n, j)
    if log_n == 5:            # the reference's own statement (linear_codes/utils.rs:303-331): encoded[j] = p(omega^j)
        w = R.root_of_unity(FR, 5)
        vals = B.fr_from_mont(got[0])
        assert vals == [R.poly_eval(FR, co[0], pow(w, j, r)) for j in range(32)]


def test_column_hash_and_merkle_tree(ctx):
    rows, cols = 5, 64
    vals = R.gen_scalars(FR, 0x377600, rows * cols)
    ext = B.fr_mont(vals).reshape(rows, cols, 4)
    for name in ("sha256", "blake2s"):
        got = ctx.column_hash(CURVE, ext, name)
        want = [R.column_digest(FR, [vals[i * cols + j] for i in range(rows)], name) for j in range(cols)]
        assert [got[j].tobytes() for j in range(cols)] == want, name
        nodes = ctx.merkle_tree(got, name)
        assert nodes.tobytes() == b"".join(R.merkle_tree(want, name, True))


def test_ligero_commit(ctx):
    """LinearCodePCS::commit of 4096 coefficients (Blake2s columns, SHA-256 tree): the copy's root, leaves and encoded matrix"""
    coeffs = R.gen_scalars(FR, 0x377700, 4096)
    st = R.ligero_commit(FR, coeffs)
    n_rows, n_cols = st["n_rows"], st["n_cols"]
    flat = coeffs + [0] * (n_rows * n_cols - len(coeffs))
    mat = B.fr_mont(flat).reshape(n_rows, n_cols, 4)
    log_n = st["n_ext_cols"].bit_length() - 1
    ext = np.zeros((n_rows, 1 << log_n, 4), dtype=np.uint64)
    nodes, leaves = ctx.ligero_commit(CURVE, mat, log_n, ext_out=ext)
    assert nodes[0].tobytes() == st["root"]
    assert [leaves[j].tobytes() for j in range(1 << log_n)] == st["leaves"]
    assert nodes.tobytes() == b"".join(st["nodes"])
    assert [B.fr_from_mont(ext[i]) for i in range(n_rows)] == st["ext"]
    assert hashlib.sha256(b"").digest() != st["root"]


def test_group_two_contexts(ctx, key, true_srs):
    """pc_hip_group_msm / pc_hip_group_kzg_open with two contexts on device 0 at n = 4097: the single-context results"""
    import poly_commit_amd as pc
    pts, words, keys = key
    beta, srs = true_srs
    n = NMAX
    g = pc.Group([0, 0])
    ks = R.gen_scalars(FR, 0x377800, n)
    for table in (False, True):
        gs = g.upload_srs(CURVE, words, precompute=table)
        got, inf = gs.msm(B.fr(ks))
        assert (got == keys["plain"].msm(B.fr(ks))[0]).all() and (got == B.point(B.closed_form(ks))).all() and not inf
        got, _ = gs.msm(B.fr_mont(ks[:2000]), base_offset=2040, montgomery=True)          # a slice across the two chunks
        assert (got == B.point(B.closed_form(ks[:2000], first=2041))).all()
        gs.free()
    powers = srs.read(0, n)
    gs = g.upload_srs(CURVE, powers)
    z = R.gen_scalars(FR, 0x377801, 1)[0]
    mont, zm = B.fr_mont(ks), B.fr_mont([z])[0]
    proof, value = gs.kzg_open(mont, zm)
    _, want_w, want_v = _open_expected(ks, z, beta)
    assert (proof == srs.kzg_open(mont, zm)[0]).all() and (proof == want_w).all() and B.fr_from_mont(value) == [want_v]
    assert (gs.msm(mont, montgomery=True)[0] == srs.msm(mont, montgomery=True)[0]).all()
    gs.free()
    g.close()


def test_g2_and_multilinear_pc_refuse_the_curve(ctx):
    """Fq2 of BLS12-377 is Fq[u] / (u^2 + 5): the G2 and MultilinearPC entry points keep PC_ERR_INVALID_ARG for the id"""
    import poly_commit_amd as pc
    with pytest.raises(pc._ffi.PcHipError) as e:
        ctx.upload_g2_srs(CURVE, np.zeros((2, 192), dtype=np.uint8))
    assert e.value.status == -1
    with pytest.raises(pc._ffi.PcHipError) as e:
        ctx.ml_setup(CURVE, 2, np.zeros(96, dtype=np.uint8), np.zeros(192, dtype=np.uint8), B.fr_mont([3, 5]))
    assert e.value.status == -1
