"""The C++ oracle's BLS12-377 (curve id 3) against the private Python copy of the reference (tests/harness/ref377.py), in Python
integers: field and curve unit operations at their boundary operands, the input generators, the MSM schedules over the edge sets the
device runs (tests/test_bls12_377_gpu.py; both take them from the harness), the NTT, the KZG pieces, the IPA rounds, serialization and the Ligero encode.

The two share the moduli and the generator (tools/gen_constants.py derives the oracle's header from the same numbers) and nothing
else: every Montgomery constant is checked here through the operations that use it.  The device tests can then hold the HIP library
against BOTH checkers, and neither shares code with it."""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from harness import ipa377
from harness import ref377 as B

R, CURVE, FQ, FR, r, p = B.R, B.CURVE, B.FQ, B.FR, B.RMOD, B.P
ID = O.CURVES[CURVE]
NMAX = 4097


def _field_op(name, which, a, b):
    """orc_f_<name> on two canonical integers, through Montgomery form and back"""
    n64, mod, rad = (6, p, B.RQ) if which == 0 else (4, r, B.RR)
    am, bm = B.limbs([a * rad % mod], n64)[0], B.limbs([b * rad % mod], n64)[0]
    out = np.zeros(n64, dtype=np.uint64)
    getattr(O.lib(), "orc_f_" + name)(ID, which, O.p64(am), O.p64(bm), O.p64(out))
    got = B.ints(out.reshape(1, n64))[0]
    assert got < mod, (name, which, hex(a), hex(b))               # results are canonical residues
    return got * pow(rad, -1, mod) % mod


@pytest.mark.parametrize("which", [0, 1])
def test_field_ops_at_boundary_operands(which):
    n64, mod, rad, field = (6, p, B.RQ, FQ) if which == 0 else (4, r, B.RR, FR)
    assert O.lib().orc_fq_limbs(ID) == 6 and O.lib().orc_fr_bits(ID) == 253 and p.bit_length() == 377
    rnd = random.Random(0x377F + which)
    vals = [0, 1, 2, mod - 1, mod - 2, rad % mod, (mod - rad) % mod, rad * rad % mod, pow(rad, -1, mod), (mod + 1) // 2, (1 << (mod.bit_length() - 1)) - 1,
            1 << (mod.bit_length() - 1)] + [rnd.randrange(mod) for _ in range(8)] + R.gen_scalars(field, 0x377F0, 4)
    for a in vals:
        for b in vals:
            assert _field_op("mul", which, a, b) == a * b % mod, (hex(a), hex(b))
            assert _field_op("add", which, a, b) == (a + b) % mod, (hex(a), hex(b))
            assert _field_op("sub", which, a, b) == (a - b) % mod, (hex(a), hex(b))
        if a:
            assert _field_op("inv", which, a, 0) == pow(a, -1, mod), hex(a)
    # to and from Montgomery form: a * R mod p, limb for limb
    canon = B.limbs(vals, n64)
    mont = O.f_to_mont(CURVE, which, canon)
    assert B.ints(mont) == [v * rad % mod for v in vals]
    assert (O.f_from_mont(CURVE, which, mont) == canon).all()
    if which == 1:
        assert (mont == B.fr_mont(vals)).all() and O.fr_from_mont_array(CURVE, mont) == vals and (O.fr_mont_array(CURVE, vals) == mont).all()


def _ec(name, P, Q):
    out = np.zeros(12, dtype=np.uint64)
    getattr(O.lib(), "orc_ec_" + name)(ID, O.p64(B.point(P)), O.p64(Q if name == "mul" else B.point(Q)), O.p64(out))
    return B.point_of(out)


def test_curve_unit_ops():
    g = np.zeros(12, dtype=np.uint64)
    O.lib().orc_generator(ID, O.p64(g))
    assert B.point_of(g) == B.G == R.generator(CURVE) and O.lib().orc_on_curve(ID, O.p64(g)) == 1
    pts, _ = B.gen_bases(9)
    P, Q = pts[4], pts[6]
    neg = R.ec_neg(CURVE, P)
    assert _ec("add", P, Q) == R.ec_add(CURVE, P, Q) == B.mul_g(12) and _ec("add", Q, P) == B.mul_g(12)
    assert _ec("add", P, P) == R.ec_add(CURVE, P, P) == B.mul_g(10)                      # the doubling branch of the mixed addition
    assert _ec("add", P, neg) is None and _ec("add", neg, P) is None
    assert _ec("add", None, Q) == Q and _ec("add", P, None) == P and _ec("add", None, None) is None
    for k in (0, 1, 2, r - 1, r, r + 1, 0x1234567 << 220, (1 << 256) - 1):
        want = R.ec_mul(CURVE, k, P)
        assert _ec("mul", P, B.limbs([k], 4)[0]) == want == B.mul_g(5 * k), hex(k)
    assert _ec("mul", P, B.limbs([r], 4)[0]) is None and _ec("mul", P, B.limbs([r - 1], 4)[0]) == neg
    assert _ec("mul", None, B.limbs([7], 4)[0]) is None
    # on_curve: the points above, their negatives, infinity; not (x, y + 1), not (x + 1, y), not a swapped pair
    for A in pts + [neg]:
        assert O.lib().orc_on_curve(ID, O.p64(B.point(A))) == 1 and R.on_curve(CURVE, A)
    for A in ((P[0], (P[1] + 1) % p), ((P[0] + 1) % p, P[1]), (P[1], P[0])):
        assert O.lib().orc_on_curve(ID, O.p64(B.point(A))) == 0 and not R.on_curve(CURVE, A)


@pytest.fixture(scope="module")
def key():
    """P_i = (i + 1) G, i < 4097: the copy's points (Python) and the oracle's words (C++), identical"""
    pts, words = B.gen_bases(NMAX)
    got = O.gen_bases(CURVE, NMAX)
    assert (got == words).all()
    return pts, words


def test_input_generators_identical_to_the_copy(key):
    pts, words = key
    for n in (1, 2, 3, 5, 64, 1000):                                  # every length is a prefix, whatever the doubling ladder's steps
        assert (O.gen_bases(CURVE, n) == words[:n]).all(), n
    assert O.array_to_points(CURVE, words[:3]) == pts[:3] and (O.points_to_array(CURVE, pts[:3] + [None]) == B.points(pts[:3] + [None])).all()
    for seed, n in ((0, 1), (0x377, 1000), (0x5EED0001, 4097), ((1 << 64) - 1, 33)):
        sc = O.gen_scalars(CURVE, seed, n)
        assert B.ints(sc) == R.gen_scalars(FR, seed, n), (seed, n)
        assert max(B.ints(sc)) < r


def _msm_all(words, sc, naive):
    out = {m: O.msm_pippenger(CURVE, words, sc, 8, m) for m in (0, 1, 2)}
    out["one thread"] = O.msm_pippenger(CURVE, words, sc, 1, 1)
    if naive:
        out["naive"] = O.msm_naive(CURVE, words, sc)
    return out


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 257, 4097])
def test_msm_schedules_over_the_edge_sets(key, n):
    """msm_naive and msm_pippenger in modes 0 (window-parallel), 1 (chunk-parallel) and 2 (the tuned port), over every edge key and edge
    scalar set of the device tests, against ONE Python scalar multiplication: sum k_i (d_i G) = (sum k_i d_i mod r) G."""
    pts, words = key
    by_dlog = lambda d: B.point(None) if d == 0 else (words[d - 1] if d > 0 else B.point(R.ec_neg(CURVE, pts[-d - 1])))
    scalars = B.edge_scalars(n, 0xED6E + n)
    keys = B.edge_keys(n) if n >= 8 else {"plain": [i + 1 for i in range(n)]}
    for kname, dl in keys.items():
        kw = np.ascontiguousarray(np.stack([by_dlog(d) for d in dl])) if n else np.zeros((0, 12), dtype=np.uint64)
        packed = {name: B.fr(ks) if n else np.zeros((0, 4), dtype=np.uint64) for name, ks in scalars.items()}
        with ThreadPoolExecutor(4) as pool:                         # the naive sums at 4097 pairs take a second each: side by side
            results = dict(zip(packed, pool.map(lambda sc: _msm_all(kw, sc, naive=True), packed.values())))
        for name, ks in scalars.items():
            want = B.point(B.mul_g(sum(k * d for k, d in zip(ks, dl))))
            for how, got in results[name].items():
                assert (got == want).all(), (n, kname, name, how)
    if n >= 8:                                                      # the whole sum cancels: P beside -P under equal scalars, an even count
        m = n - n % 2
        dl = B.edge_keys(m)["P beside -P"]
        kw = np.ascontiguousarray(np.stack([by_dlog(d) for d in dl]))
        for how, got in _msm_all(kw, B.fr(B.edge_scalars(m, 5)["equal in pairs"]), naive=True).items():
            assert not got.any(), (n, how)


def test_msm_min_len_and_python_naive(key):
    pts, words = key
    ks = R.gen_scalars(FR, 0x377000, 64)
    want = B.point(R.msm(CURVE, pts[:64], ks))
    assert (O.msm_naive(CURVE, words[:64], B.fr(ks)) == want).all() and (want == B.point(B.closed_form(ks))).all()
    assert (O.msm_pippenger(CURVE, words[:40], B.fr(ks), 8, 1) == B.point(B.closed_form(ks[:40]))).all()      # min(len) pairs
    assert (O.msm_pippenger(CURVE, np.ascontiguousarray(words[100:]), B.fr(ks), 8, 2) == B.point(B.closed_form(ks, first=101))).all()


@pytest.mark.parametrize("log_n", range(13))
def test_ntt_and_roots_of_unity(log_n):
    N = 1 << log_n
    w = O.fr_from_mont_array(CURVE, O.root_of_unity(CURVE, log_n).reshape(1, 4))[0]
    assert w == R.root_of_unity(FR, log_n) and pow(w, N, r) == 1 and (N == 1 or pow(w, N // 2, r) == r - 1)
    rows = 3
    for in_cols in sorted({1, N, max(1, N // 2), max(1, N - 1), max(1, (N // 4) * 3 + (1 if N > 4 else 0))}):            # ragged: zero-padded rows
        co = [R.gen_scalars(FR, 0x377500 + 16 * log_n + j + in_cols, in_cols) for j in range(rows)]
        mat = np.stack([B.fr_mont(c) for c in co])
        got = O.ntt_batch(CURVE, mat, log_n)
        assert got.shape == (rows, N, 4)
        for j in range(rows):
            assert B.fr_from_mont(got[j]) == R.ntt(FR, co[j], log_n), (log_n, in_cols, j)
    if log_n <= 5:                                                  # the reference's own statement: out[j] = p(omega^j)
        assert B.fr_from_mont(got[0]) == [R.poly_eval(FR, co[0], pow(w, j, r)) for j in range(N)]
    # more columns than the domain: the tail is ignored
    if log_n == 3:
        wide = np.stack([B.fr_mont(R.gen_scalars(FR, 5, 11))])
        assert (O.ntt_batch(CURVE, wide, 3) == O.ntt_batch(CURVE, np.ascontiguousarray(wide[:, :8]), 3)).all()


def test_two_adic_root_is_the_one_the_device_header_holds():
    top = O.fr_from_mont_array(CURVE, O.root_of_unity(CURVE, 47).reshape(1, 4))[0]
    assert top == R.two_adic_root(FR) == pow(B.FR_GEN, (r - 1) >> 47, r) and R.two_adicity(r) == 47 and R.two_adicity(p) == 46


@pytest.fixture(scope="module")
def srs(key):
    """beta^i G, i < 301, in words, with beta"""
    beta = R.gen_scalars(FR, 0xBE7A377, 1)[0]
    pw = [pow(beta, i, r) for i in range(301)]
    return beta, np.ascontiguousarray(np.stack([B.point(B.mul_g(k)) for k in pw]))


@pytest.mark.parametrize("n,lead,trail", [(1, 0, 0), (2, 0, 0), (300, 0, 0), (300, 5, 0), (301, 17, 9), (40, 40, 0), (33, 0, 32)])
def test_kzg_pieces(srs, n, lead, trail):
    """poly_eval, witness_poly, kzg_commit (leading zero coefficients skipped by offsetting the powers, kzg10/mod.rs:452-461; trailing
    ones lower the degree, :393-403) and kzg_open: commit = p(beta) G and open = q(beta) G on the true SRS"""
    beta, powers = srs
    coeffs = R.gen_scalars(FR, 0x377400 + n, n)
    coeffs[:lead] = [0] * lead
    if trail:
        coeffs[n - trail:] = [0] * trail
    z = R.gen_scalars(FR, 0x377401, 1)[0]
    mont, zm = B.fr_mont(coeffs), B.fr_mont([z])[0]
    assert B.fr_from_mont(O.poly_eval(CURVE, mont, zm)) == [R.poly_eval(FR, coeffs, z)]
    q = R.witness_polynomial(FR, coeffs, z)
    assert B.fr_from_mont(O.witness_poly(CURVE, mont, zm)) == q[:n - 1] + [0] * (n - 1 - len(q))
    rc, comm = O.kzg_commit(CURVE, powers, mont)
    assert rc == 0 and (comm == B.point(B.mul_g(R.poly_eval(FR, coeffs, beta)))).all()
    rc, proof = O.kzg_open(CURVE, powers, mont, zm)
    assert rc == 0 and (proof == B.point(B.mul_g(R.poly_eval(FR, q, beta)))).all()
    if n <= 40:                                                     # the copy's own commit / open, point arithmetic in Python
        pts = O.array_to_points(CURVE, powers[:n])
        assert B.point_of(comm) == R.kzg_commit(CURVE, pts, coeffs) and B.point_of(proof) == R.kzg_open(CURVE, pts, coeffs, z)
    # the verifier's equation with the known trapdoor: C - v G = (beta - z) W
    v = R.poly_eval(FR, coeffs, z)
    lhs = R.ec_add(CURVE, B.point_of(comm), R.ec_neg(CURVE, B.mul_g(v)) if v else None)
    assert lhs == R.ec_mul(CURVE, (beta - z) % r, B.point_of(proof))


def test_kzg_commit_refuses_too_many_coefficients(srs):
    beta, powers = srs
    mont = B.fr_mont(R.gen_scalars(FR, 3, 302))
    assert O.kzg_commit(CURVE, powers, mont)[0] == -1
    mont[301] = 0                                                   # degree 300: 301 coefficients, fits
    assert O.kzg_commit(CURVE, powers, mont)[0] == 0


@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_ipa_rounds_against_the_logarithms(n):
    """orc_ipa_rounds on a key with known logarithms (an infinity among them) against tests/harness/ipa377.py's restatement in Fr"""
    rnd = random.Random(0x1FA + n)
    d = [rnd.randrange(1, r) for _ in range(n)]
    if n >= 8:
        d[3] = 0
    h_log = rnd.randrange(1, r)
    coeffs = R.gen_scalars(FR, 0x377900 + n, n)
    if n >= 8:
        coeffs[5] = 0
    z = R.gen_scalars(FR, 0x377901, 1)[0]
    lg = n.bit_length() - 1
    ch = [rnd.randrange(1, r) for _ in range(max(lg, 1))]
    l_logs, r_logs, key_log, c = ipa377.ipa_rounds_dlog(d, h_log, coeffs, z, ch)
    key = ipa377.log_points(d)
    l, rr, fk, cc = O.ipa_rounds(CURVE, key, B.fr_mont(coeffs), B.fr_mont([z])[0], B.point(B.mul_g(h_log)), B.fr_mont(ch))
    assert B.fr_from_mont(cc) == [c] and (fk == ipa377.log_points([key_log])[0]).all()
    if lg:
        assert (l == ipa377.log_points(l_logs)).all() and (rr == ipa377.log_points(r_logs)).all()
    if n == 8:                                                      # and the copy's ipa_rounds itself, points in Python
        want = R.ipa_rounds(CURVE, [B.mul_g(x) if x else None for x in d], coeffs, z, B.mul_g(h_log), ch)
        assert [B.point_of(x) for x in l] == list(want[0]) and [B.point_of(x) for x in rr] == list(want[1])
        assert B.point_of(fk) == want[2] and c == want[3]


def test_ipa_fiat_shamir_challenges_use_the_generic_point_bytes():
    """the transcript of the rounds hashes ser(L) || ser(R): the challenges the oracle derives are the copy's over ITS bytes"""
    n = 4
    d = [3, 5, 7, 11]
    key = ipa377.log_points(d)
    coeffs = R.gen_scalars(FR, 0x377A00, n)
    z, rc0 = R.gen_scalars(FR, 0x377A01, 2)
    l, rr, fk, c, ch = O.ipa_rounds_fs(CURVE, key, B.fr_mont(coeffs), B.fr_mont([z])[0], B.point(B.mul_g(13)), B.fr_mont([rc0])[0])
    cur, got = rc0, B.fr_from_mont(ch)
    for j in range(2):
        cur = R.random_oracle_challenge(FR, R.ser_field(FR, cur) + R.ser_point(CURVE, B.point_of(l[j])) + R.ser_point(CURVE, B.point_of(rr[j])))
        assert got[j] == cur, j
    first = O.ipa_first_challenge(CURVE, key[1], B.fr_mont([z])[0], B.fr_mont([rc0])[0])
    assert B.fr_from_mont(first) == [R.random_oracle_challenge(FR, R.ser_point(CURVE, B.mul_g(5)) + R.ser_field(FR, z) + R.ser_field(FR, rc0))]


def test_ser_point_is_the_generic_short_weierstrass_form():
    """NOT BLS12-381's zcash form: x then y little-endian, 48 bytes each, 0x80 in the last byte when y > -y, 0x40 for infinity"""
    pts, _ = B.gen_bases(9)
    larger = lambda A: A if A[1] > p - A[1] else R.ec_neg(CURVE, A)
    for A in (larger(pts[3]), R.ec_neg(CURVE, larger(pts[4])), pts[0], R.ec_neg(CURVE, pts[0]), None):
        got = O.ser_point(CURVE, B.point(A))
        assert got == R.ser_point(CURVE, A) and len(got) == 96
        if A is None:
            assert got == bytes(95) + b"\x40"
        else:
            assert got[:48] == A[0].to_bytes(48, "little") and got[95] & 0x80 == (0x80 if A[1] > p - A[1] else 0)
            assert int.from_bytes(got[48:95] + bytes([got[95] & 0x3F]), "little") == A[1]
            # the compressed mode is the same x with the same flags: the copy writes it, the oracle's flags agree
            comp = R.ser_point_compressed(CURVE, A)
            assert comp[:47] == got[:47] and comp[47] & 0xC0 == got[95] & 0xC0
    assert R.ser_point_compressed(CURVE, None)[47] == 0x40 == O.ser_point(CURVE, B.point(None))[95]


def test_ligero_encode():
    """compute_matrices (linear_codes/mod.rs:118-138): the zero-padded row-major matrix, every row through the NTT"""
    poly_len = 3000
    coeffs = R.gen_scalars(FR, 0x377700, poly_len)
    n_rows, n_cols, t = O.ligero_dims(253, poly_len)
    st = R.ligero_commit(FR, coeffs)
    assert (n_rows, n_cols) == (st["n_rows"], st["n_cols"])
    ext = O.ligero_encode(CURVE, B.fr_mont(coeffs), n_rows, n_cols)
    assert ext.shape[1] == st["n_ext_cols"]
    assert [B.fr_from_mont(ext[i]) for i in range(n_rows)] == st["ext"]


def test_the_three_earlier_curves_keep_their_ids_and_the_reference_its_three():
    import pyref
    assert [O.CURVES[c] for c in ("bls12_381", "bn254", "pallas")] == [0, 1, 2] and sorted(pyref.CURVES) == ["bls12_381", "bn254", "pallas"]
    assert O.ref("bn254") is pyref and O.ref(CURVE) is R and R is not pyref
    assert [O.lib().orc_fq_limbs(i) for i in range(4)] == [6, 4, 4, 6] and [O.lib().orc_fr_bits(i) for i in range(4)] == [255, 254, 255, 253]
