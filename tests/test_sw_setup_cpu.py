"""sample_generators over the short Weierstrass curves without a GPU: the Python restatement (tests/harness/sw_setup.py) against the
facts of the curves, the generated constants (csrc/setup_constants.h) against tools/gen_constants.py and those facts, and the kernel
bodies of csrc/sw_setup.hpp as compiled by g++ (the host build of tests/hip/probe_sw_setup.hip) against the restatement on the boundary
sets of tests/harness/swsetupprobe.py."""
import importlib.util
import os
import re

import pytest

from harness import sw_setup as S
from harness import swsetupprobe as P

R = S.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = S.CURVES


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def test_cofactors():
    """the published cofactors of the two BLS12 G1 groups; 1 for BN254 and Pallas"""
    assert S.cofactor("bls12_381") == 0x396c8c005555e1568c00aaab0000aaab
    assert S.cofactor("bls12_377") == 0x170b5d44300000000000000000000000
    assert S.cofactor("bn254") == 1 and S.cofactor("pallas") == 1


def test_jacobian_ladder_is_the_affine_one():
    for curve in CURVES:
        G = R.generator(curve)
        for k in (1, 2, 3, 5, 0xdeadbeef, R.curve_params(curve)[1] - 1):
            assert S.mul(curve, k, G) == R.ec_mul(curve, k, G)
        assert S.mul(curve, R.curve_params(curve)[1], G) is R.INF


@pytest.mark.parametrize("curve", CURVES)
def test_generators_lie_in_the_group(curve):
    """64 generators per curve: on the curve, r G = infinity, pairwise distinct"""
    r = R.curve_params(curve)[1]
    pts, counts = S.generators(curve, S.IPA_NAME, 0, 64)
    assert all(q is not R.INF and R.on_curve(curve, q) for q in pts)
    assert all(S.mul(curve, r, q) is R.INF for q in pts)
    assert len(set(pts)) == 64 and min(counts) >= 1


@pytest.mark.parametrize("curve", CURVES)
def test_retry_branch_is_taken(curve):
    """among 512 indices one needed at least three digests and one exactly one: a device test against these counts cannot pass with a
    retry branch that is never taken (checked on the restatement alone)"""
    counts = [S.digest_count(curve, S.IPA_NAME, i) for i in range(512)]
    assert max(counts) >= 3 and min(counts) == 1
    # acceptance per digest: about 0.5 (BLS), 0.25 (Pallas: half the x are >= p), 0.19 (BN254: the flags as well)
    rate = 512 / sum(counts)
    lo, hi = {"bls12_381": (0.42, 0.58), "bls12_377": (0.42, 0.58), "pallas": (0.2, 0.3), "bn254": (0.14, 0.24)}[curve]
    assert lo < rate < hi, rate


def test_root_choice_is_the_deserialiser_s():
    """pick_root gives the root the project's compressed encoding names with the same flag (oracle/pyref.py): BN254's (1, 2) has the
    smaller root 2, encoded without the YIsNegative bit"""
    p = S.field("bn254")[0]
    assert S.pick_root(p, 2, False) == 2 and S.pick_root(p, p - 2, False) == 2 and S.pick_root(p, 2, True) == p - 2
    assert R.ser_point_compressed("bn254", (1, 2))[-1] & 0x80 == 0 and R.ser_point_compressed("bn254", (1, p - 2))[-1] & 0x80 == 0x80
    for curve in ("bn254", "pallas", "bls12_377"):
        pp = S.field(curve)[0]
        for i in range(8):
            g, h, _ = S.trace(curve, S.IPA_NAME, i)
            neg = (g[0], pp - g[1])
            flag = h[31] & 0x80 if curve == "bn254" else 0                 # beyond the digest elsewhere: clear, YIsPositive
            assert R.ser_point_compressed(curve, g)[-1] & 0x80 == flag
            assert R.ser_point_compressed(curve, neg)[-1] & 0x80 == 0x80 - flag


def test_bn254_flags():
    p = S.field("bn254")[0]
    low, _ = P.straddlers("bn254")
    y = S.sqrt("bn254", S.rhs("bn254", low))
    assert S.try_bytes("bn254", P.le32(low)) == (S.ACCEPT, (low, min(y, p - y)))
    assert S.try_bytes("bn254", P.le32(low | 1 << 255)) == (S.ACCEPT, (low, max(y, p - y)))
    assert S.try_bytes("bn254", P.le32(low | 1 << 254)) == (S.FLAGS, None)
    assert S.try_bytes("bn254", P.le32(low | 3 << 254)) == (S.FLAGS, None)
    assert S.try_bytes("bn254", P.le32(1 << 254)) == (S.ACCEPT, R.INF)
    assert S.try_bytes("bn254", P.le32(p)) == (S.RANGE, None)
    # Pallas: bit 255 is beyond the 255-bit coordinate and masked away; the flag byte is byte 32, outside the digest
    lowp, _ = P.straddlers("pallas")
    assert S.try_bytes("pallas", P.le32(lowp | 1 << 255)) == S.try_bytes("pallas", P.le32(lowp))


def test_setup_and_trim_shapes():
    pp = S.ipa_setup("pallas", 5)
    assert pp["max_degree"] == 7 and len(pp["comm_key"]) == 8
    gens = S.generators("pallas", S.IPA_NAME, 0, 10)[0]
    assert pp["comm_key"] == gens[:8] and pp["s"] == gens[8] and pp["h"] == gens[9]
    ck = S.ipa_trim(pp, 2)
    assert ck["supported_degree"] == 3 and ck["comm_key"] == gens[:4] and ck["h"] == gens[9]
    with pytest.raises(ValueError, match="TrimmingDegreeTooLarge"):
        S.ipa_trim(pp, 8)
    hy = S.hyrax_setup("bls12_377", 4)
    assert len(hy["com_key"]) == 4 and hy["h"] == S.generators("bls12_377", S.HYRAX_NAME, 0, 5)[0][4]
    for bad in (None, 3):
        with pytest.raises(ValueError, match="InvalidNumberOfVariables"):
            S.hyrax_setup("bls12_377", bad)


def test_python_setup_argument_errors_need_no_device():
    from poly_commit_amd import setup as D
    for bad in (None, 1, 5):
        with pytest.raises(ValueError, match="InvalidNumberOfVariables"):
            D.hyrax_setup(None, "bls12_377", bad)
    with pytest.raises(ValueError, match="TrimmingDegreeTooLarge"):
        D.ipa_trim(dict(max_degree=7), 8)


# ---- the generated constants ---------------------------------------------------------------------------------------------------------

def _gen_constants():
    spec = importlib.util.spec_from_file_location("_gen_constants_sw", os.path.join(ROOT, "tools", "gen_constants.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)      # an import writes nothing
    return m


def test_setup_constants_header_is_current():
    g = _gen_constants()
    assert open(os.path.join(ROOT, "poly_commit_amd", "csrc", "setup_constants.h")).read() == g.render_setup()


def test_setup_constants_against_the_fields():
    text = open(os.path.join(ROOT, "poly_commit_amd", "csrc", "setup_constants.h")).read()

    def words(block, name):
        m = re.search(name + r"\[\d+\] = \{([^}]*)\}", block)
        return sum(int(w.strip().rstrip("u"), 16) << (32 * k) for k, w in enumerate(m.group(1).split(",")))
    for curve in CURVES:
        fq = R.CURVES[curve]["fq"]
        p, _, n = S.field(curve)
        block = text[text.index("pc_sqrt_constants<pc_%s>" % fq):]
        block = block[:block.index("\n};")]
        s = int(re.search(r"SQRT_S = (\d+)", block).group(1))
        assert s == R.two_adicity(p)
        exp = words(block, "SQRT_EXP")
        assert exp.bit_length() == int(re.search(r"SQRT_EXP_BITS = (\d+)", block).group(1))
        t = (p - 1) >> s
        assert exp == ((p + 1) // 4 if s == 1 else (t - 1) // 2)
        c = S.unmont(curve, words(block, "SQRT_C"))
        assert pow(c, 1 << (s - 1), p) == p - 1                       # order exactly 2^s
        cb = text[text.index("pc_cofactor_constants<pc_curve_%s>" % curve):]
        cb = cb[:cb.index("\n};")]
        assert words(cb, "COFACTOR") == S.cofactor(curve)
        assert int(re.search(r"COFACTOR_BITS = (\d+)", cb).group(1)) == S.cofactor(curve).bit_length()


# ---- the host build of the probe -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    return P.host_probe()


@pytest.mark.parametrize("curve", CURVES)
def test_host_sqrt(host, curve):
    assert P.check_sqrt(host, host, curve) == P.sqrt_lanes(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_host_from_random_bytes(host, curve):
    assert P.check_try(host, host, curve) == P.try_lanes(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_host_cofactor(host, curve):
    assert P.check_cofactor(host, host, curve) == P.cofactor_lanes(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_host_sample_body(host, curve):
    assert P.check_sample(host, host, curve) == 64 + 2


def test_host_probe_refuses_an_unknown_curve(host):
    import ctypes as C
    for entry in ("pc_probe_sw_setup_sqrt", "pc_probe_sw_setup_try", "pc_probe_sw_setup_cofactor"):
        assert host.raw(entry, C.c_int(4), C.c_size_t(0), None, None) == -2
