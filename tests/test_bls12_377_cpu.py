"""BLS12-377 without a GPU: the generated constants against Python integers, the curve id in every binding, the private copy of the
Python reference (tests/harness/ref377.py), and the field / curve primitives of the new instantiations through the host build of
the probe (the CPU twin of tests/test_bls12_377_primitives_gpu.py)."""
import os
import re

import pytest

import pyref
from harness import ref377 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poly_commit_amd", "csrc")
R = B.R


def _struct(header, name):
    src = open(os.path.join(CSRC, header)).read()
    i = src.index("struct %s {" % name)
    return src[i:src.index("\n};", i)]


def _words(body, field):
    m = re.search(r"\b%s\[\d+\]\s*=\s*\{([^}]*)\}" % field, body)
    w = [int(x.strip().rstrip("ul"), 16) for x in m.group(1).split(",")]
    bits = 64 if "ull" in m.group(1) else 32
    return sum(v << (bits * i) for i, v in enumerate(w)), len(w)


def _int(body, field):
    return int(re.search(r"\b%s = (0x[0-9a-f]+|\d+)" % field, body).group(1), 0)


@pytest.mark.parametrize("name,p,gen,n", [("bls12_377_fq", B.P, B.FQ_GEN, 12), ("bls12_377_fr", B.RMOD, B.FR_GEN, 8)])
def test_field_constants(name, p, gen, n):
    body = _struct("field_constants.h", "pc_" + name)
    Rm = 1 << (32 * n)
    s = R.two_adicity(p)
    assert _int(body, "N") == n and _int(body, "BITS") == p.bit_length() and _int(body, "TWO_ADICITY") == s
    assert s == (46 if n == 12 else 47)
    assert _words(body, "MOD") == (p, n)
    assert _int(body, "INV") == (-pow(p, -1, 1 << 32)) % (1 << 32)
    assert _words(body, "ONE") == (Rm % p, n)
    assert _words(body, "R2") == (Rm * Rm % p, n)
    root = _words(body, "ROOT")[0] * pow(Rm, -1, p) % p
    assert root == pow(gen, (p - 1) >> s, p)
    assert pow(root, 1 << s, p) == 1 and pow(root, 1 << (s - 1), p) == p - 1          # exact order 2^s: the generator is a non-residue
    assert R.two_adic_root(name) == root


def test_curve_constants():
    body = _struct("field_constants.h", "pc_curve_bls12_377")
    Rq = 1 << 384
    assert "typedef pc_bls12_377_fq FqP;" in body and "typedef pc_bls12_377_fr FrP;" in body
    assert _int(body, "B_SMALL") == 1
    assert _words(body, "B_MONT") == (Rq % B.P, 12)
    assert _words(body, "GX") == (B.GX * Rq % B.P, 12) and _words(body, "GY") == (B.GY * Rq % B.P, 12)
    assert R.on_curve(B.CURVE, B.G) and R.ec_mul(B.CURVE, B.RMOD, B.G) is None
    # R = 2^384 is 152 p: the lazily reduced accumulation and its stores (fp32.hpp LAZY_OK / LAZY_FUSED_OK / LAZY_STORE_OK, all from the modulus)
    assert (1 << 384) // B.P == 152
    assert pow(15, (B.P - 1) // 2, B.P) == B.P - 1 and pow(-5, (B.P - 1) // 2, B.P) == B.P - 1 and B.P % 4 == 1


def test_glv_constants():
    body = _struct("glv_constants.h", "pc_glv_bls12_377")
    lam, _ = _words(body, "LAMBDA")
    beta = _words(body, "BETA_MONT")[0] * pow(1 << 384, -1, B.P) % B.P
    assert (lam * lam + lam + 1) % B.RMOD == 0 and 1 < lam < B.RMOD
    assert pow(beta, 3, B.P) == 1 and beta != 1
    assert R.ec_mul(B.CURVE, lam, B.G) == (beta * B.GX % B.P, B.GY)                      # phi(G) = lambda G
    # the lattice basis: a_i + b_i lambda = 0 (mod r), and the decomposition csrc/glv.hpp performs on scalars at the ends of the range
    sg = lambda f: -_words(body, f)[0] if _int(body, f + "_NEG") else _words(body, f)[0]
    a1, b1, a2, b2 = sg("A1"), sg("B1"), sg("A2"), sg("B2")
    assert (a1 + b1 * lam) % B.RMOD == 0 and (a2 + b2 * lam) % B.RMOD == 0 and abs(a1 * b2 - a2 * b1) == B.RMOD
    g1, g2 = _words(body, "G1")[0], _words(body, "G2")[0]
    n1neg, n2neg = (int(x) for x in re.search(r"N1_NEG = (\d), N2_NEG = (\d)", body).groups())
    for k in (0, 1, 2, B.RMOD - 1, B.RMOD - 2, B.RMOD // 2, lam, B.RMOD - lam, (1 << 252) - 1, 1 << 252):
        c1, c2 = (g1 * k) >> 384, (g2 * k) >> 384
        c1, c2 = (-c1 if n1neg else c1), (-c2 if n2neg else c2)
        k1, k2 = k - c1 * a1 - c2 * a2, -c1 * b1 - c2 * b2
        assert (k1 + k2 * lam - k) % B.RMOD == 0 and abs(k1).bit_length() <= 130 and abs(k2).bit_length() <= 130, hex(k)


def test_curve_id_in_every_binding():
    import poly_commit_amd._ffi as F
    header = open(os.path.join(ROOT, "include", "pc_hip.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\} pc_curve;", header).group(1)
    ids = {k.strip(): int(v) for k, v in (x.split("=") for x in enum.split(","))}
    assert ids == {"PC_CURVE_BLS12_381": 0, "PC_CURVE_BN254": 1, "PC_CURVE_PALLAS": 2, "PC_CURVE_BLS12_377": 3}
    assert F.CURVES == {"bls12_381": 0, "bn254": 1, "pallas": 2, "bls12_377": 3} and F.FQ_BYTES["bls12_377"] == 48
    rs = open(os.path.join(ROOT, "rust", "poly-commit-hip", "src", "ffi.rs")).read()
    assert re.search(r"pub const PC_CURVE_BLS12_377: c_int = 3;", rs)
    curve_rs = open(os.path.join(ROOT, "rust", "poly-commit-hip", "src", "curve.rs")).read()
    assert "ark_bls12_377::g1::Config, ark_bls12_377::Fq, 6, ffi::PC_CURVE_BLS12_377" in curve_rs
    assert "ark_bls12_377::Fr, ffi::PC_CURVE_BLS12_377" in curve_rs
    from poly_commit_amd import ipa, sharded
    assert sharded.FR_MODULUS["bls12_377"] == B.RMOD and ipa.FQ_MODULUS["bls12_377"] == B.P
    bound = open(os.path.join(CSRC, "curves.hpp")).read()
    assert "PC_CURVE_LAST = PC_CURVE_BLS12_377" in bound


def test_private_copy_leaves_the_reference_alone():
    assert list(pyref.CURVES) == ["bls12_381", "bn254", "pallas"] and len(pyref.FIELDS) == 6
    assert R is not pyref and B.CURVE in R.CURVES and B.FR in R.FIELDS and B.FQ in R.FIELDS
    assert B.probe().R is R
    from harness import probe
    assert probe.R is pyref and B.probe() is not probe


def test_private_copy_computes_the_curve():
    pts, words = B.gen_bases(64)
    assert pts[0] == B.G and all(R.on_curve(B.CURVE, A) for A in pts[:5]) and words.shape == (64, 12)
    assert B.point_of(words[5]) == pts[5] and B.point_of(B.point(None)) is None
    ks = R.gen_scalars(B.FR, 0x377, 64)
    assert R.msm(B.CURVE, pts, ks) == B.closed_form(ks)
    assert B.fr_from_mont(B.fr_mont(ks)) == ks
    # ark-ec's generic short-Weierstrass encoding: 96 / 48 bytes, flags in the top bits of the last byte
    A = pts[1] if pts[1][1] > B.P - pts[1][1] else R.ec_neg(B.CURVE, pts[1])
    assert len(R.ser_point(B.CURVE, A)) == 96 and len(R.ser_point_compressed(B.CURVE, A)) == 48
    assert R.ser_point(B.CURVE, A)[-1] & 0x80 and R.ser_point_compressed(B.CURVE, None)[-1] == 0x40
    # reed_solomon as the reference pins it (linear_codes/utils.rs:303-331): encoded[j] = p(omega^j)
    co = R.gen_scalars(B.FR, 5, 8)
    w = R.root_of_unity(B.FR, 5)
    assert R.ntt(B.FR, co, 5) == [R.poly_eval(B.FR, co, pow(w, j, B.RMOD)) for j in range(32)]


# ---- the primitives of the new instantiations, host build of the probe (the device runs the same cases) ---------------------------

@pytest.fixture(scope="module")
def host():
    return B.probe().host_probe()


@pytest.mark.parametrize("group", ["products", "fused", "additive", "inv", "lazy_products", "lazy_fused", "lazy_additive"])
@pytest.mark.parametrize("field", [B.FQ, B.FR])
def test_field(host, field, group):
    assert B.probe().check_field(host, host, field, group) > 0


@pytest.mark.parametrize("group", ["add_affine", "add", "dbl", "add_affine_lz"])
def test_curve(host, group):
    assert B.probe().check_curve(host, host, B.CURVE, group) > 0


def test_lazy_flags_come_from_the_modulus(host):
    """Fq: R = 152 p, so the accumulation is lazily reduced (LAZY_OK), its fused pair needs no subtraction (R >= 8p) and its sums
    are stored as they are (R >= 9p); Fr: 2^256 = 13.7 r."""
    P = B.probe()
    for name in (B.FQ, B.FR):
        f = P.Field(name)
        assert f.lazy and f.lazy_fused
        assert host.raw("pc_probe_field_lazy_bls12_377", P.C.c_int(f.which)) == 3
    assert host.raw("pc_probe_field_lazy_store_bls12_377", P.C.c_int(0)) == 1


# ---- the checkers of the IPA / protocol GPU tests (tests/harness/ipa377.py, tests/harness/brakedown.py on the fourth field) --------

@pytest.mark.parametrize("n,zero_at", [(2, None), (4, 2), (16, None), (16, 9)])
def test_ipa_rounds_over_logarithms_equal_the_copy_on_points(n, zero_at):
    """ipa_rounds_dlog's logarithms times G are R.ipa_rounds on the real points P_i = d_i G, d_i = i + 1 -- one case per size with a
    generator at infinity (d_i = 0)"""
    from harness import ipa377 as I
    pts, _ = B.gen_bases(n + 1)
    d = [i + 1 for i in range(n)]
    key = list(pts[:n])
    if zero_at is not None:
        d[zero_at], key[zero_at] = 0, None
    h_log = n + 1
    coeffs = R.gen_scalars(B.FR, 0x1A0 + n, n)
    coeffs[n // 2] = 0
    z = R.gen_scalars(B.FR, 0x1A1, 1)[0]
    ch = R.gen_scalars(B.FR, 0x1A2 + n, n.bit_length() - 1)
    want_l, want_r, want_key, want_c = R.ipa_rounds(B.CURVE, key, coeffs, z, pts[n], ch)
    l, r_, k, c = I.ipa_rounds_dlog(d, h_log, coeffs, z, ch)
    g = lambda e: B.mul_g(e) if e else None                                  # noqa: E731
    assert [g(e) for e in l] == want_l and [g(e) for e in r_] == want_r and g(k) == want_key and c == want_c
    assert (I.log_points(l) == B.points(want_l)).all()


def test_fold_case_is_the_fold_of_its_key():
    """fold_case: the expected points (an addition chain, special lanes by mul_g) are K_l[i] + u K_r[i] of the key its logarithms
    describe, computed the slow way on points"""
    from harness import ipa377 as I
    half = 12
    for u in (0, 1, B.RMOD - 1, I.glv_constants()["lam"], 0x1234567 << 200):
        specials = dict(zip((1, 3, 5, 7, 9), I.SPECIAL_LANES))
        d, want, e, delta = I.fold_case(half, u, 0xF0 + half, specials)
        assert e[2] == (e[0] + 2 * delta) % B.RMOD and e[9] == 0
        pts = [B.mul_g(x) if x else None for x in d]
        assert pts[1] is None and pts[half + 3] is None and pts[5] is None and pts[half + 5] is None
        got = [R.ec_add(B.CURVE, pts[i], R.ec_mul(B.CURVE, u, pts[half + i]) if u else None) for i in range(half)]
        assert got == want, hex(u)
        assert want[9] is None and (u == 0 or want[7] == R.ec_add(B.CURVE, pts[7], pts[7]))
    d, want, _, _ = I.fold_case(5, 7, 1, inf_lo=1, inf_hi=2)
    assert d[1] == 0 and d[5 + 2] == 0 and want[2] == B.mul_g(d[2]) and want[1] == B.mul_g(7 * d[5 + 1])
    some, zeros = I.check_positions(d)
    assert some[0] == 0 and some[-1] == 9 and len(some) == 4 and zeros == [1, 7]


def test_glv_split_in_python_and_the_longest_split():
    """glv_split restates glv_decompose (the same arithmetic as test_glv_constants); the seeded search for the challenge with the
    longest halves finds 127 bits -- inside GLV_HALF_BITS = 130 and the fold table's 131 rows (NAF digits at bits 0 .. 127)"""
    from harness import ipa377 as I
    g = I.glv_constants()
    lam = g["lam"]
    assert (lam * lam + lam + 1) % B.RMOD == 0
    for name, k in I.edge_challenges():
        k1, k2 = I.glv_split(k, g)
        assert (k1 + k2 * lam - k) % B.RMOD == 0 and max(abs(k1), abs(k2)).bit_length() <= 130, name
    k, bits = I.longest_split()
    assert bits == 127 and 0 < k < B.RMOD
    assert max(abs(x) for x in I.glv_split(k, g)).bit_length() == 127
    # The basis of this curve puts every split on one side.  With truncated quotients the remainder is f1 v1 + f2 v2, f1, f2 in [0, 1),
    # of the basis vectors v1 = (a1, b1) = (1, -|b1|), v2 = (a2, b2) = (|a2|, 1): k1 = f1 + f2 |a2| >= 0, and k2 = f2 - f1 |b1| < 1 is an
    # integer, so k2 <= 0.  EcFoldGlvBody's neg1 is therefore never set on this curve, and neg2 whenever k2 != 0 -- asserted for the
    # edge challenges and the 4000 seeded values.
    assert g["a1"] == 1 and g["b1"] < 0 and g["a2"] > 0 and g["b2"] == 1
    assert all(k1 >= 0 >= k2 for k1, k2 in (I.glv_split(k, g) for k in [u for _, u in I.edge_challenges()] + I.seeded_challenges()))
    # the other curves' constants parse the same way (the edge-challenge fold test runs on BLS12-381 and Pallas too)
    for curve, fr in (("bls12_381", "bls12_381_fr"), ("pallas", "pallas_fr")):
        p = pyref.FIELDS[fr]["p"]
        gc = I.glv_constants(curve)
        assert (gc["lam"] ** 2 + gc["lam"] + 1) % p == 0
        for name, k in I.edge_challenges(p, curve):
            k1, k2 = I.glv_split(k, gc)
            assert 0 <= k < p and (k1 + k2 * gc["lam"] - k) % p == 0 and max(abs(k1), abs(k2)).bit_length() <= 130, (curve, name)


def test_brakedown_harness_on_the_fourth_field():
    """tests/harness/brakedown.py with BLS12-377's Fr: the modulus comes from the private copy, the encode is linear and systematic,
    the clipped concurrent form equals the reference's loop, the base code is its definition, and the kernel bodies of csrc/sprs.hpp
    instantiated for pc_bls12_377_fr and stepped lane by lane give the same codewords -- rows of all r - 1 and all 0 included"""
    from harness import brakedown as BD
    import test_brakedown_cpu as TB
    assert BD.FIELD_ID[B.CURVE] == 3 and BD.field_p(B.CURVE) == B.RMOD and BD.ref_of(B.CURVE) is R and BD.ref_of("bn254") is pyref
    p = B.RMOD
    _, code = BD.default_code(B.CURVE, 10, 0x377B)
    assert code.p == p and all(0 < v < p for mt in code.a_mats + code.b_mats for v in mt.val)
    x, y = BD.messages(code, 2, 31)
    a, b = BD.Gen(77).nonzero(p), BD.Gen(78).nonzero(p)
    ex, ey = BD.encode(code, x), BD.encode(code, y)
    assert ex[:code.m] == x and len(ex) == code.m_ext
    assert BD.encode(code, [(a * u + b * v) % p for u, v in zip(x, y)]) == [(a * u + b * v) % p for u, v in zip(ex, ey)]
    levels = list(range(len(code.start)))
    assert BD.encode(code, x, b_order=levels[::-1], clip=True) == ex
    base = BD.base_code(B.CURVE, 17)
    m17 = BD.messages(base, 1, 5)[0]
    assert BD.encode(base, m17) == [sum(c * pow(k, i, p) for i, c in enumerate(m17)) % p for k in range(1, 27)]
    for cd in (code, BD.ragged_code(B.CURVE), base):
        msgs = BD.messages(cd, 3, 9) + [[p - 1] * cd.m, [0] * cd.m]
        want = [BD.encode(cd, m) for m in msgs]
        assert want[-1] == [0] * cd.m_ext
        assert TB.emu_encode(cd, msgs) == want, cd.m
    # the commitment's digests go through the copy's column_digest (the field's byte length)
    st = BD.ref_commit(base, 2, m17 + m17)
    assert st["leaves"][3] == R.column_digest(B.FR, [st["ext"][0][3], st["ext"][1][3]], "blake2s")
