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
