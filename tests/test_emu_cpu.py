"""CPU suite, part 2: the product's 32-bit-limb field / curve code (host compilation of
csrc/fp32.hpp, csrc/ec.hpp) and the MSM / division-scan orchestration (csrc/msm.hpp,
csrc/poly.hpp) stepped lane by lane by tests/emu, against the independent 64-bit oracle.
This validates the indexing logic of the kernels on a machine without a GPU; the GPU suite
(-m gpu) validates the same code as compiled for gfx950, through the C ABI."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = ["bls12_381", "bn254", "pallas"]
_emu = None


def emu():
    global _emu
    if _emu is None:
        # PC_EMU_SANITIZE=1 (tools/emu_sanitize.sh): the same bodies under AddressSanitizer + UBSan -- the sanitizer run the GPU pool cannot do
        san = os.environ.get("PC_EMU_SANITIZE") == "1"
        so = os.path.join(HERE, "emu", "libemu_san.so" if san else "libemu.so")
        srcs = [os.path.join(HERE, "emu", "emu_msm.cpp")] + [
            os.path.join(HERE, "..", "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "poly.hpp", "ec.hpp", "fp32.hpp", "ipa.hpp", "g2.hpp", "glv.hpp", "serialize.hpp", "fold_table.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
            tmp = "%s.%d.tmp" % (so, os.getpid())                      # (xdist workers may build at once: each its own file, renamed into place)
            subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def run_msm(curve, b, s, c=0, T=0, T2=0, K0=0, base_off=0, from_mont=0):
    out = np.zeros(2 * O.fq_limbs(curve), dtype=np.uint64)
    emu().emu_msm(O.CURVES[curve], p32(b.view(np.uint32)), p32(s.view(np.uint32)), C.c_size_t(len(s)), base_off, c, T, T2,
                  K0, from_mont, p32(out.view(np.uint32)))
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_field_ops_32bit_vs_bigint(curve):
    rnd = random.Random(7)
    ci = O.CURVES[curve]
    for which, fname in ((0, R.CURVES[curve]["fq"]), (1, R.CURVES[curve]["fr"])):
        p = R.FIELDS[fname]["p"]
        n64 = R.FIELDS[fname]["limbs64"]
        Rm = 1 << (64 * n64)
        Ri = pow(Rm, -1, p)
        vals = [0, 1, p - 1, 2, p - 2, Rm % p] + [rnd.randrange(p) for _ in range(20)]
        for op in range(5):
            for _ in range(25):
                a, b = rnd.choice(vals), rnd.choice(vals)
                A, B = O.ints_to_limbs([a], n64)[0], O.ints_to_limbs([b], n64)[0]
                out = np.zeros(n64, dtype=np.uint64)
                emu().emu_fop(ci, which, op, p32(A.view(np.uint32)), p32(B.view(np.uint32)), p32(out.view(np.uint32)))
                got = O.limbs_to_ints(out.reshape(1, -1))[0]
                want = [a * b * Ri % p, (a + b) % p, (a - b) % p, (pow(a * Ri % p, -1, p) * Rm % p) if a else 0,
                        (-a) % p][op]
                assert got == want, (fname, op, a, b)


@pytest.mark.parametrize("ci,fname,n64", [(0, "bls12_381_fq", 6), (1, "bn254_fq", 4)])
def test_lazy_reduction_helpers(ci, fname, n64):
    """The mod-2p helpers behind the lazily reduced bucket accumulation (fp32.hpp LAZY_OK: BLS12-381 Fq with R >= 8p, BN254 Fq
    with 4p <= R < 8p, where the fused pair keeps one conditional subtraction), on inputs anywhere in [0, 2p] including the
    boundary representatives 0, p, 2p.  The host forms skip the final subtraction exactly where the device's do, so the raw
    outputs (ops 19-21) show the real ranges."""
    p = R.FIELDS[fname]["p"]
    Rm = 1 << (64 * n64)
    assert 4 * p <= Rm
    Ri = pow(Rm, -1, p)
    rnd = random.Random(11)
    vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p] + [rnd.randrange(2 * p + 1) for _ in range(30)]

    def run(op, a, b=0):
        A, B = O.ints_to_limbs([a], n64)[0], O.ints_to_limbs([b], n64)[0]
        out = np.zeros(n64, dtype=np.uint64)
        emu().emu_fop(ci, 0, op, p32(A.view(np.uint32)), p32(B.view(np.uint32)), p32(out.view(np.uint32)))
        return O.limbs_to_ints(out.reshape(1, -1))[0]
    for a in vals:
        assert run(14, a) == a % p                                        # canon
        assert run(15, a) == (1 if a % p == 0 else 0)                     # is_zero_lz
        assert run(12, a) == 2 * p - a                                    # neg_lz: no zero special case
        if a < 2 * p:
            d = run(11, a)
            assert d < 2 * p and d % p == 2 * a % p                       # dbl_lz
        if a < p:
            assert run(13, a) == p - a                                    # neg_lz_canonical
        assert run(17, a) == a * a * Ri % p                               # sqr_lz
        raw = run(20, a)
        assert raw < 2 * p and raw % p == a * a * Ri % p and (raw * Rm - a * a) % p == 0
        for b in vals:
            s = run(10, a, b)
            assert 0 <= s <= 2 * p and (s - (a - b)) % p == 0 and (a == 2 * p or s < 2 * p)   # sub_lz stays in range
            assert run(16, a, b) == a * b * Ri % p                        # mul_lz
            assert run(18, a, b) == (a * b + b * a) * Ri % p              # fused pair
            raw = run(19, a, b)
            assert raw < 2 * p and raw % p == a * b * Ri % p
            # Montgomery's quotient is determined by the product alone: the raw value is exactly (a b + m p) / R
            m = (-a * b * pow(p, -1, Rm)) % Rm
            assert raw == (a * b + m * p) // Rm
            raw = run(21, a, b)
            assert raw < 2 * p and raw % p == 2 * a * b * Ri % p


@pytest.mark.parametrize("curve", CURVES)
def test_xyzz_group_law_all_special_cases(curve):
    pts = R.gen_bases(curve, 5)
    arr = O.points_to_array(curve, pts + [None])
    for i in range(6):
        for j in range(6):
            Pi = pts[i] if i < 5 else None
            Pj = pts[j] if j < 5 else None
            for op in range(4):
                out = np.zeros(arr.shape[1], dtype=np.uint64)
                emu().emu_ecop(O.CURVES[curve], op, p32(arr[i].view(np.uint32)), p32(arr[j].view(np.uint32)),
                               p32(out.view(np.uint32)))
                want = R.ec_add(curve, Pi, Pj) if op < 2 else R.ec_add(curve, Pi, Pi)
                assert O.array_to_points(curve, out)[0] == want, (op, i, j)
            if curve in ("bls12_381", "bn254"):        # the lazily reduced mixed addition (same special cases; op 5 negates twice; op 6 chains three)
                for op, want in ((4, R.ec_add(curve, Pi, Pj)), (5, R.ec_add(curve, Pi, Pj)), (6, R.ec_add(curve, Pi, Pj))):
                    out = np.zeros(arr.shape[1], dtype=np.uint64)
                    emu().emu_ecop(O.CURVES[curve], op, p32(arr[i].view(np.uint32)), p32(arr[j].view(np.uint32)), p32(out.view(np.uint32)))
                    assert O.array_to_points(curve, out)[0] == want, ("lazy", op, i, j)
    # P + (-P) through the mixed add
    neg = O.points_to_array(curve, [R.ec_neg(curve, pts[2])])[0]
    out = np.ones(arr.shape[1], dtype=np.uint64)
    emu().emu_ecop(O.CURVES[curve], 0, p32(arr[2].view(np.uint32)), p32(neg.view(np.uint32)), p32(out.view(np.uint32)))
    assert not out.any()


@pytest.mark.parametrize("curve", CURVES)
def test_two_lane_addition_stepped(curve):
    """The XYZZ addition spread over a lane pair (k_bucket_level_coop2; ec.hpp HalfAdd): both lanes stepped on the host through the
    device's own phases -- every pair of {5 points, infinity}, with trivial and non-trivial ZZ on either side (so P + P, P + (-P)
    and both infinities are in it): equal to the group law AND coordinate-for-coordinate to the one-lane XyzzD::add."""
    pts = R.gen_bases(curve, 5)
    pts.append(R.ec_neg(curve, pts[1]))
    arr = O.points_to_array(curve, pts + [None])
    nq = arr.shape[1]
    for i in range(7):
        for j in range(7):
            Pi = pts[i] if i < 6 else None
            Pj = pts[j] if j < 6 else None
            for mode in range(4):
                out = np.zeros(nq + 1, dtype=np.uint64)
                emu().emu_half_add(O.CURVES[curve], mode, p32(arr[i].view(np.uint32)), p32(arr[j].view(np.uint32)), p32(out.view(np.uint32)))
                assert O.array_to_points(curve, out[:nq].reshape(1, -1))[0] == R.ec_add(curve, Pi, Pj), (mode, i, j)
                assert out.view(np.uint32)[2 * nq] == 1, ("coordinates differ from XyzzD::add", mode, i, j)


@pytest.mark.parametrize("curve", CURVES)
def test_msm_pipeline_stepped(curve):
    for n in (1, 2, 33, 300):
        b = O.gen_bases(curve, n)
        s = O.gen_scalars(curve, n * 7 + 1, n)
        want = O.msm_pippenger(curve, b, s, 4, 1)
        # the last three use "bits" reduction levels (fan-in >= 16): at level 0 with weights l+1, then
        # twice in a row (older arrays folded by a bits level), then bits followed by a serial level
        for (c, T, T2, K0) in ((0, 0, 0, 0), (4, 3, 4, 2), (5, 1, 4, 4), (7, 16, 16, 8), (8, 5, 5, 2), (2, 2, 4, 2),
                               (11, 4, 8, 4), (7, 0, 0, 0), (9, 5, 4, 16), (10, 0, 0, 0)):
            assert (run_msm(curve, b, s, c, T, T2, K0) == want).all(), (n, c, T, T2, K0)


def test_msm_stepped_adversarial_scalars():
    """Bucket collisions / huge buckets / signed-digit carries: the cases SURVEY.md 7 calls out."""
    curve = "bls12_381"
    n = 400
    r = R.FIELDS["bls12_381_fr"]["p"]
    b = O.gen_bases(curve, n)
    b[5] = 0                 # infinity among the bases
    b[11] = b[10]            # repeated base -> doubling inside a bucket
    rnd = O.gen_scalars(curve, 3, n)
    cases = {
        "zeros": np.zeros((n, 4), dtype=np.uint64),
        "ones": O.ints_to_limbs([1] * n, 4),
        "r-1": O.ints_to_limbs([r - 1] * n, 4),
        "same": np.ascontiguousarray(np.repeat(rnd[:1], n, axis=0)),     # one bucket per window holds everything
        "two-values": np.ascontiguousarray(np.where((np.arange(n) % 2 == 0)[:, None], rnd[:1], rnd[1:2])),
        "carry-chain": O.ints_to_limbs([(1 << 254) - 1 - i for i in range(n)], 4),
        "sparse": np.ascontiguousarray(np.where((np.arange(n) % 7 == 0)[:, None], rnd, 0).astype(np.uint64)),
    }
    for name, sc in cases.items():
        want = O.msm_naive(curve, b, sc)
        for (c, T, T2, K0) in ((0, 0, 0, 0), (6, 4, 4, 2), (9, 7, 5, 4)):
            assert (run_msm(curve, b, sc, c, T, T2, K0) == want).all(), (name, c, T)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_msm_stepped_equal_partial_sums_meet_in_the_joins(curve):
    """ONE base repeated under ONE scalar: every chunk of a bucket's run sums to the same point, so the segmented reduction (and
    the bucket reduction behind it) adds equal multi-entry partial sums -- XyzzD::add takes its doubling branch on coordinates
    that left the accumulation lazily reduced (BLS12-381: in [0, 2p), fp32.hpp LAZY_STORE_OK; BN254: canonical at the flush).
    Round-3 advisor finding: dbl()'s U = 2Y is not a product, its headroom is now stated and asserted."""
    n = 64
    g = O.gen_bases(curve, 3)
    b = np.ascontiguousarray(np.repeat(g[2:3], n, axis=0))
    k = O.gen_scalars(curve, 5, 1)
    for sc in (np.ascontiguousarray(np.repeat(k, n, axis=0)), O.ints_to_limbs([1] * n, 4), O.ints_to_limbs([3] * n, 4)):
        want = O.msm_naive(curve, b, sc)
        for (c, T, T2, K0) in ((4, 4, 4, 2), (6, 8, 4, 2), (5, 2, 4, 4), (7, 16, 4, 2), (3, 1, 4, 2)):
            assert (run_msm(curve, b, sc, c, T, T2, K0) == want).all(), (c, T)


@pytest.mark.parametrize("n_srs,n", [(1024, 1023), (1024, 512), (1024, 31), (2048, 2047), (33, 31), (300, 255)])
def test_msm_plan_sized_for_srs_serves_shorter_calls(n_srs, n):
    """A plan is sized once per SRS; a call just below a power of two runs with the smaller window of its
    bracket, i.e. with MORE digits per scalar than any power-of-two length (the KZG open shape: n - 1 pairs
    over a 2^k SRS).  The workspace must cover it (round-1 advisor finding: it did not)."""
    curve = "bn254"
    b = O.gen_bases(curve, n_srs)
    s = O.gen_scalars(curve, 11 + n, n)
    out = np.zeros(2 * O.fq_limbs(curve), dtype=np.uint64)
    rc = emu().emu_msm_sized(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(n_srs), p32(s.view(np.uint32)), C.c_size_t(n),
                             n_srs - n, 0, p32(out.view(np.uint32)))
    assert rc == 0, "the plan refused a call within its SRS length"
    assert (out == O.msm_pippenger(curve, np.ascontiguousarray(b[n_srs - n:]), s, 4, 1)).all()


def test_msm_stepped_offset_and_montgomery():
    curve = "bn254"
    n = 200
    b = O.gen_bases(curve, n)
    s = O.gen_scalars(curve, 5, n)
    want = O.msm_naive(curve, b[50:], s[:150])
    assert (run_msm(curve, b, np.ascontiguousarray(s[:150]), 6, 4, 4, 4, base_off=50) == want).all()
    mont = O.f_to_mont(curve, 1, s)
    assert (run_msm(curve, b, mont, 0, 0, 0, 0, from_mont=1) == O.msm_naive(curve, b, s)).all()


def run_msm_table(curve, b, s, c, K0=0, base_off=0, from_mont=0):
    out = np.zeros(2 * O.fq_limbs(curve), dtype=np.uint64)
    emu().emu_msm_table(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(len(b)), p32(s.view(np.uint32)), C.c_size_t(len(s)),
                        base_off, c, K0, from_mont, p32(out.view(np.uint32)))
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_msm_window_table_mode_stepped(curve):
    """pc_hip_srs_precompute: table[w][i] = 2^(c w) P_i, all digits into one shared bucket set --
    same point as the table-free MSM, incl. a base offset (powers_of_g[lz..]), infinity and
    repeated bases, all-(r-1) scalars (carry into the top digit) and Montgomery input."""
    n = 150
    r = R.FIELDS[curve + "_fr"]["p"]
    b = O.gen_bases(curve, n)
    b[5] = 0
    b[11] = b[10]
    s = O.gen_scalars(curve, 17, n)
    want = O.msm_naive(curve, b, s)
    for c, K0 in ((4, 2), (7, 0), (9, 16), (12, 4), (16, 0)):
        assert (run_msm_table(curve, b, s, c, K0) == want).all(), (c, K0)
    top = O.ints_to_limbs([r - 1] * n, 4)
    assert (run_msm_table(curve, b, top, 8) == O.msm_naive(curve, b, top)).all()
    assert (run_msm_table(curve, b, np.ascontiguousarray(s[:100]), 6, 2, base_off=50) == O.msm_naive(curve, b[50:], s[:100])).all()
    assert (run_msm_table(curve, b, O.f_to_mont(curve, 1, s), 10, 0, from_mont=1) == want).all()
    assert not run_msm_table(curve, b, np.zeros((n, 4), dtype=np.uint64), 5).any()


def run_msm_table_glv(curve, b, s, c, K0=0, base_off=0, from_mont=0):
    out = np.zeros(2 * O.fq_limbs(curve), dtype=np.uint64)
    emu().emu_msm_table_glv(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(len(b)), p32(s.view(np.uint32)), C.c_size_t(len(s)),
                            base_off, c, K0, from_mont, p32(out.view(np.uint32)))
    return out


GLV_LAMBDA = {"bls12_381": 0xac45a4010001a40200000000ffffffff,
              "bn254": 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd,
              "pallas": 0x06819a58283e528e511db4d81cf70f5a0fed467d47c033af2aa9d2e050aa0e4f}


@pytest.mark.parametrize("curve", CURVES)
def test_glv_split_32bit_limbs(curve):
    """GlvHalves::split (what the MSM's digit passes run on the device): k = +-|k1| +- |k2| lambda (mod r) with both magnitudes below
    2^130 (GLV_HALF_BITS: six windows of 22 bits), identical to the 64-bit host decomposition -- on random, small, and extreme
    scalars.  lambda from glv_constants.h: lambda^2 + lambda + 1 = 0 (mod r)."""
    r = R.FIELDS[R.CURVES[curve]["fr"]]["p"]
    lam = GLV_LAMBDA[curve]
    assert (lam * lam + lam + 1) % r == 0
    rnd = random.Random(5)
    ks = [0, 1, 2, r - 1, r - 2, lam, lam + 1, r - lam, (1 << 128) - 1, 1 << 128, (1 << 200) + 12345, r >> 1] + [rnd.randrange(r) for _ in range(300)]
    worst = 0
    for k in ks:
        kin = O.ints_to_limbs([k], 4)[0]
        out = np.zeros(12, dtype=np.uint32)
        same = emu().emu_glv_split(O.CURVES[curve], p32(kin.view(np.uint32)), p32(out))
        assert same == 1, hex(k)
        k1 = sum(int(out[i]) << (32 * i) for i in range(5)); k2 = sum(int(out[5 + i]) << (32 * i) for i in range(5))
        s1 = -1 if out[10] else 1; s2 = -1 if out[11] else 1
        assert (s1 * k1 + s2 * k2 * lam - k) % r == 0, hex(k)
        worst = max(worst, k1.bit_length(), k2.bit_length())
    assert worst <= 129, worst


@pytest.mark.parametrize("curve", CURVES)
def test_msm_glv_table_mode_stepped(curve):
    """The GLV form of the window table (MsmGeom::glv): the table holds the windows of the 130-bit halves only, the digits of k1 go to
    bucket set 0 and those of k2 to set 1 with the SAME table point, phi is applied once to the reduced sum of set 1.  Same point as
    the naive MSM: offsets, infinity and repeated bases, edge scalars (the halves' signs, zero halves, r - 1), Montgomery input,
    cooperative and serial reduction plans."""
    n = 150
    r = R.FIELDS[curve + "_fr"]["p"]
    lam = GLV_LAMBDA[curve]
    b = O.gen_bases(curve, n)
    b[5] = 0
    b[11] = b[10]
    s = O.gen_scalars(curve, 17, n)
    want = O.msm_naive(curve, b, s)
    for c, K0 in ((4, 2), (7, 0), (9, 16), (12, 4), (16, 0), (22, 0)):
        assert (run_msm_table_glv(curve, b, s, c, K0) == want).all(), (c, K0)
    edge = [0, 1, 2, r - 1, r - 2, lam % r, (lam + 1) % r, (r - lam) % r, (1 << 127), (1 << 128) - 1, (1 << 129) + 7, r >> 1, 3 * lam % r, (lam * lam) % r]
    sc = O.ints_to_limbs([edge[i % len(edge)] for i in range(n)], 4)
    assert (run_msm_table_glv(curve, b, sc, 8) == O.msm_naive(curve, b, sc)).all()
    assert (run_msm_table_glv(curve, b, sc, 13, 4) == O.msm_naive(curve, b, sc)).all()
    top = O.ints_to_limbs([r - 1] * n, 4)
    assert (run_msm_table_glv(curve, b, top, 8) == O.msm_naive(curve, b, top)).all()
    assert (run_msm_table_glv(curve, b, np.ascontiguousarray(s[:100]), 6, 2, base_off=50) == O.msm_naive(curve, b[50:], s[:100])).all()
    assert (run_msm_table_glv(curve, b, O.f_to_mont(curve, 1, s), 10, 0, from_mont=1) == want).all()
    assert not run_msm_table_glv(curve, b, np.zeros((n, 4), dtype=np.uint64), 5).any()
    same = np.ascontiguousarray(np.repeat(s[:1], n, axis=0))
    assert (run_msm_table_glv(curve, b, same, 6, 2) == O.msm_naive(curve, b, same)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_msm_many_mode_stepped(curve):
    """pc_hip_msm_many (Hyrax's one-MSM-per-matrix-row, hyrax/mod.rs:233-242): B MSMs over the same m
    bases in one pass -- sub-MSM s owns bucket set s of the shared table pipeline; results folded per
    sub-MSM and batch-normalised.  Rows that are all zero give infinity."""
    m, B = 40, 7
    b = O.gen_bases(curve, m)
    b[3] = b[2]
    s = O.gen_scalars(curve, 99, B * m).reshape(B, m, 4)
    s[4] = 0
    s[5, :, :] = s[5, :1, :]
    want = np.stack([O.msm_naive(curve, b, np.ascontiguousarray(s[k])) for k in range(B)])
    assert not want[4].any()
    for c, K0 in ((4, 2), (6, 0), (8, 4), (11, 0)):
        out = np.zeros((B, 2 * O.fq_limbs(curve)), dtype=np.uint64)
        flat = np.ascontiguousarray(s.reshape(B * m, 4))
        emu().emu_msm_many(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(m), p32(flat.view(np.uint32)), C.c_size_t(B), c, K0, 0,
                           p32(out.view(np.uint32)))
        assert (out == want).all(), (c, K0)
    mont = O.f_to_mont(curve, 1, np.ascontiguousarray(s.reshape(B * m, 4)))
    out = np.zeros((B, 2 * O.fq_limbs(curve)), dtype=np.uint64)
    emu().emu_msm_many(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(m), p32(mont.view(np.uint32)), C.c_size_t(B), 5, 0, 1,
                       p32(out.view(np.uint32)))
    assert (out == want).all()


@pytest.mark.parametrize("curve", CURVES)
def test_division_scan_stepped(curve):
    for n in (1, 2, 3, 64, 65, 130, 1000):
        for G in (2, 3, 64):
            co = O.gen_scalars(curve, n, n)
            z = O.gen_scalars(curve, 999, 1)[0]
            want = O.witness_poly(curve, co, z)
            q = np.zeros((max(n - 1, 1), 4), dtype=np.uint64)
            emu().emu_witness(O.CURVES[curve], p32(co.view(np.uint32)), C.c_size_t(n), p32(z.view(np.uint32)),
                              p32(q.view(np.uint32)), G)
            assert (q[: max(n - 1, 0)] == want).all(), (n, G)
    # with a carry-in: equals the scan of the concatenation [chunk | higher chunk]
    n = 300
    full = O.gen_scalars(curve, 1, 2 * n)
    z = O.gen_scalars(curve, 2, 1)[0]
    whole = np.zeros((2 * n, 4), dtype=np.uint64)
    emu().emu_div_scan(O.CURVES[curve], p32(full.view(np.uint32)), C.c_size_t(2 * n), p32(z.view(np.uint32)), None,
                       p32(whole.view(np.uint32)), 64)
    lo = np.zeros((n, 4), dtype=np.uint64)
    low_half = np.ascontiguousarray(full[:n])
    carry = np.ascontiguousarray(whole[n])          # value after element n = carry into the low chunk
    emu().emu_div_scan(O.CURVES[curve], p32(low_half.view(np.uint32)), C.c_size_t(n), p32(z.view(np.uint32)),
                       p32(carry.view(np.uint32)), p32(lo.view(np.uint32)), 64)
    assert (lo == whole[:n]).all()


@pytest.mark.parametrize("curve", CURVES)
def test_poly_eval_stepped(curve):
    """pc_hip_poly_eval's level structure (the up-sweep of the division scan alone) == Horner evaluation
    with Python integers, for lengths around the chunk sizes and two fan-ins."""
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    zi = R.gen_scalars(fr, 0xE7A1, 1)[0]
    z = O.fr_mont_array(curve, [zi])[0]
    for n in (1, 2, 7, 8, 9, 63, 64, 65, 129, 1000):
        ci = R.gen_scalars(fr, 0xE7A2 + n, n)
        want = 0
        for c in reversed(ci):
            want = (want * zi + c) % p
        co = O.fr_mont_array(curve, ci)
        for G in (16, 4):
            out = np.zeros(4, dtype=np.uint64)
            emu().emu_poly_eval(O.CURVES[curve], p32(co.view(np.uint32)), C.c_size_t(n), p32(z.view(np.uint32)), p32(out.view(np.uint32)), G)
            assert O.fr_from_mont_array(curve, out.reshape(1, 4))[0] == want, (n, G)


@pytest.mark.parametrize("curve", ["pallas", "bls12_381"])
def test_ipa_round_bodies_stepped(curve):
    """fr_fold / fr_dot / ec_fold / fr_powers (ipa_pc/mod.rs:641-649, 672-707) vs Python big ints."""
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    half = 5
    pts = R.gen_bases(curve, 2 * half)
    key = O.points_to_array(curve, pts)
    u = R.gen_scalars(fr, 1, 1)[0]
    lo_i, hi_i = R.gen_scalars(fr, 2, half), R.gen_scalars(fr, 3, half)
    s_i, z_i = R.gen_scalars(fr, 4, 2)
    lo, hi = O.fr_mont_array(curve, lo_i), O.fr_mont_array(curve, hi_i)
    s_m, z_m = O.fr_mont_array(curve, [s_i])[0], O.fr_mont_array(curve, [z_i])[0]
    u_c = O.ints_to_limbs([u], 4)[0]
    dot = np.zeros(4, dtype=np.uint64)
    npow = 37
    pw = np.zeros((npow, 4), dtype=np.uint64)
    emu().emu_ipa_bodies(O.CURVES[curve], p32(key.view(np.uint32)), C.c_size_t(half), p32(u_c.view(np.uint32)),
                         p32(lo.view(np.uint32)), p32(hi.view(np.uint32)), p32(s_m.view(np.uint32)), p32(dot.view(np.uint32)),
                         p32(z_m.view(np.uint32)), p32(pw.view(np.uint32)), C.c_size_t(npow))
    assert O.array_to_points(curve, key[:half]) == [R.ec_add(curve, pts[i], R.ec_mul(curve, u, pts[half + i])) for i in range(half)]
    assert O.fr_from_mont_array(curve, dot.reshape(1, 4))[0] == sum(a * b for a, b in zip(lo_i, hi_i)) % p
    assert O.fr_from_mont_array(curve, lo) == [(a + s_i * b) % p for a, b in zip(lo_i, hi_i)]
    assert O.fr_from_mont_array(curve, pw) == [pow(z_i, k, p) for k in range(npow)]


@pytest.mark.parametrize("curve", CURVES)
def test_naf_jacobian_scalar_mul_stepped(curve):
    """The two per-lane ladders against Python big ints, including the scalars whose NAF carries out of the top limb: NAF recoding +
    Jacobian ladder (csrc/ec.hpp JacD / NafMasks, what the key fold runs; stepped through FixedBaseMulBody), and the double-and-add
    over XYZZ with its normalisation that the fixed-base multiplication runs below its table threshold."""
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    G = R.gen_bases(curve, 3)[2]
    ks = [0, 1, 2, 3, 7, p - 1, p - 2, (1 << 254) - 1 if p > (1 << 254) else (1 << 253) - 1, 0xAAAAAAAAAAAAAAAA, 0xFFFFFFFFFFFFFFFFFFFFFFFF] + \
        R.gen_scalars(fr, 21, 6)
    ks = [k % p for k in ks]
    sc = O.fr_mont_array(curve, ks)
    g = O.points_to_array(curve, [G])[0]
    want = [R.ec_mul(curve, k, G) for k in ks]
    for ladder in (emu().emu_fixed_base_naf, emu().emu_fixed_base):
        out = np.zeros((len(ks), 2 * O.fq_limbs(curve)), dtype=np.uint64)
        ladder(O.CURVES[curve], p32(g.view(np.uint32)), p32(sc.view(np.uint32)), C.c_size_t(len(ks)), p32(out.view(np.uint32)))
        assert O.array_to_points(curve, out) == want


def _column_digests_hashlib(curve, ext_mont, hash_name):
    """FieldToBytesColHasher<F, D> (bench-templates/src/lib.rs:309-338) with Python's hashlib:
    D(u64_le(len) || 32-byte LE canonical residues of the column)."""
    import hashlib
    rows, n_cols = ext_mont.shape[0], ext_mont.shape[1]
    canon = O.f_from_mont(curve, 1, np.ascontiguousarray(ext_mont.reshape(-1, 4))).reshape(rows, n_cols, 4)
    out = []
    for j in range(n_cols):
        h = hashlib.new(hash_name)
        h.update(rows.to_bytes(8, "little"))
        h.update(np.ascontiguousarray(canon[:, j, :]).tobytes())      # little-endian u64 limbs = LE bytes
        out.append(h.digest())
    return out


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("rows", [1, 2, 3, 7, 8, 64])
def test_column_hash_stepped_vs_hashlib(curve, rows):
    n_cols = 5
    ext = O.f_to_mont(curve, 1, O.gen_scalars(curve, 300 + rows, rows * n_cols)).reshape(rows, n_cols, 4)
    for hid, name in ((0, "sha256"), (1, "blake2s")):
        out = np.zeros((n_cols, 8), dtype=np.uint32)
        emu().emu_column_hash(O.CURVES[curve], p32(np.ascontiguousarray(ext).view(np.uint32)), rows, n_cols, hid, p32(out))
        want = _column_digests_hashlib(curve, ext, name)
        assert [out[j].tobytes() for j in range(n_cols)] == want, (curve, rows, name)


@pytest.mark.parametrize("curve", CURVES)
def test_glv_split_and_fold_stepped(curve):
    """GLV: k = (+-k1) + (+-k2)*lambda mod r with short k1, k2 (csrc/glv.hpp glv_decompose), and the
    Shamir/NAF ladder of the IPA key fold (EcFoldGlvBody) against Python big ints."""
    fr = R.CURVES[curve]["fr"]
    r = R.FIELDS[fr]["p"]
    lam = np.zeros(4, dtype=np.uint64)
    emu().emu_glv_lambda(O.CURVES[curve], O.p64(lam))
    lam = O.limbs_to_ints(lam.reshape(1, 4))[0]
    assert (lam * lam + lam + 1) % r == 0
    half = 3
    pts = R.gen_bases(curve, 2 * half)
    for k in [0, 1, 2, r - 1, r - 2, lam, (lam + 1) % r, (1 << 200) + 12345] + R.gen_scalars(fr, 31, 8):
        key = O.points_to_array(curve, pts)
        split = np.zeros(12, dtype=np.uint32)
        kc = O.ints_to_limbs([k], 4)[0]
        emu().emu_glv_fold(O.CURVES[curve], p32(key.view(np.uint32)), C.c_size_t(half), O.p64(kc), p32(split))
        k1 = sum(int(split[i]) << (32 * i) for i in range(5)) * (-1 if split[10] else 1)
        k2 = sum(int(split[5 + i]) << (32 * i) for i in range(5)) * (-1 if split[11] else 1)
        assert (k1 + k2 * lam - k) % r == 0 and abs(k1).bit_length() <= 130 and abs(k2).bit_length() <= 130
        assert O.array_to_points(curve, key[:half]) == [R.ec_add(curve, pts[i], R.ec_mul(curve, k, pts[half + i])) for i in range(half)]


@pytest.mark.parametrize("curve", CURVES)
def test_glv_fold_with_batched_normalisation_stepped(curve):
    """EcFoldGlvBody leaving Jacobian results + JacBatchAffineBody (one inversion per K points, Montgomery's
    trick -- normalize_batch of ipa_pc/mod.rs:706-708), including an infinity result inside a batch."""
    fr = R.CURVES[curve]["fr"]
    r = R.FIELDS[fr]["p"]
    half = 7
    pts = R.gen_bases(curve, 2 * half)
    k = R.gen_scalars(fr, 77, 1)[0]
    pts[2] = R.ec_neg(curve, R.ec_mul(curve, k, pts[half + 2]))      # key[2] + k * key[half + 2] = infinity
    pts[half + 4] = None                                             # infinity among the inputs
    for K in (1, 3, 4, 16):
        key = O.points_to_array(curve, pts)
        emu().emu_glv_fold_batched(O.CURVES[curve], p32(key.view(np.uint32)), C.c_size_t(half), O.p64(O.ints_to_limbs([k], 4)[0]), K)
        assert O.array_to_points(curve, key[:half]) == [R.ec_add(curve, pts[i], R.ec_mul(curve, k, pts[half + i])) for i in range(half)], K


@pytest.mark.parametrize("curve", CURVES)
def test_ipa_fixed_key_rounds_stepped(curve):
    """The late halving rounds without folding the key (pc_hip_ipa_key_scalars): with s the per-base factors,
    MSM(K0, out_l) / MSM(K0, out_r) are the round's key-side sums and MSM(K0, s) is the folded key."""
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    n0 = 8
    K0 = R.gen_bases(curve, n0)
    key = list(K0)
    cs = R.gen_scalars(fr, 0x51, n0)
    s = O.fr_mont_array(curve, [1] * n0)
    ci = O.CURVES[curve]
    m = n0
    for u in R.gen_scalars(fr, 0x52, 3):
        h = m // 2
        c_arr = O.fr_mont_array(curve, cs[:m])
        out_l, out_r = np.zeros((n0, 4), dtype=np.uint64), np.zeros((n0, 4), dtype=np.uint64)
        emu().emu_ipa_key_scalars(ci, p32(c_arr.view(np.uint32)), m, p32(s.view(np.uint32)), n0, None, 0, p32(out_l.view(np.uint32)), p32(out_r.view(np.uint32)))
        assert R.msm(curve, K0, O.fr_from_mont_array(curve, out_l)) == R.msm(curve, key[:h], cs[h:m])
        assert R.msm(curve, K0, O.fr_from_mont_array(curve, out_r)) == R.msm(curve, key[h:m], cs[:h])
        # the fold, on the real key and on the factors
        ui = pow(u, -1, p)
        for i in range(h):
            cs[i] = (cs[i] + ui * cs[h + i]) % p
            key[i] = R.ec_add(curve, key[i], R.ec_mul(curve, u, key[h + i]))
        u_m = O.fr_mont_array(curve, [u])[0]
        emu().emu_ipa_key_scalars(ci, None, 0, p32(s.view(np.uint32)), n0, p32(u_m.view(np.uint32)), m, None, None)
        m = h
        assert [R.msm(curve, [K0[j] for j in range(n0) if j % m == i], [O.fr_from_mont_array(curve, s)[j] for j in range(n0) if j % m == i])
                for i in range(m)] == key[:m]
    assert R.msm(curve, K0, O.fr_from_mont_array(curve, s)) == key[0]


@pytest.mark.parametrize("curve", CURVES)
def test_check_polynomial_coefficients_from_key_folds_stepped(curve):
    """The verifier's final-key MSM (InnerProductArgPC::check, ipa_pc/mod.rs:759-765) takes
    SuccinctCheckPolynomial::compute_coeffs (data_structures.rs:204-220).  The host layers build them on the device by
    folding a vector of ones by every round challenge at sizes n, n/2, ... (IpaKeyScalarUpdateBody, stepped here):
    the same 2^log_d coefficients."""
    fr = R.CURVES[curve]["fr"]
    ci = O.CURVES[curve]
    for log_d in (1, 3, 5):
        n = 1 << log_d
        chal = R.gen_scalars(fr, 0x60 + log_d, log_d)
        s = O.fr_mont_array(curve, [1] * n)
        m = n
        for u in chal:
            u_m = O.fr_mont_array(curve, [u])[0]
            emu().emu_ipa_key_scalars(ci, None, 0, p32(s.view(np.uint32)), n, p32(u_m.view(np.uint32)), m, None, None)
            m //= 2
        assert O.fr_from_mont_array(curve, s) == R.succinct_check_coeffs(fr, chal)


@pytest.mark.parametrize("curve,compressed", [("bls12_381", False), ("bls12_381", True), ("bn254", False), ("bn254", True), ("pallas", False),
                                              ("pallas", True)])
def test_srs_decode_ark_serialize_stepped(curve, compressed):
    """CanonicalDeserialize of Vec<G1Affine> (the head of kzg10::UniversalParams, kzg10/data_structures.rs:80-112): the
    device decoder (SrsDecodeBody, stepped on the CPU) against the Python big-int serialiser -- both roots, infinity,
    and a corrupted point is counted as invalid."""
    pts = R.gen_bases(curve, 6)
    pts[1] = R.ec_neg(curve, pts[1])
    pts[4] = None
    data = R.ser_g1_vec(curve, pts, compressed)
    body = np.frombuffer(data[8:], dtype=np.uint8).copy()
    assert int.from_bytes(data[:8], "little") == 6
    out = np.zeros((6, 2 * O.fq_limbs(curve)), dtype=np.uint64)
    bad = emu().emu_srs_decode(O.CURVES[curve], body.ctypes.data_as(C.POINTER(C.c_uint8)), 6, 1 if compressed else 0, p32(out.view(np.uint32)))
    assert bad == 0 and O.array_to_points(curve, out) == pts
    # ... and the encoder (SrsEncodeBody) writes exactly those bytes back (CanonicalSerialize of the points)
    enc = np.zeros(len(body), dtype=np.uint8)
    emu().emu_srs_encode(O.CURVES[curve], p32(out.view(np.uint32)), 6, 1 if compressed else 0, enc.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert bytes(enc) == bytes(body)
    # flip a low bit of the first x: (almost surely) no longer a point
    body2 = body.copy()
    body2[47 if curve == "bls12_381" else 0] ^= 1
    bad = emu().emu_srs_decode(O.CURVES[curve], body2.ctypes.data_as(C.POINTER(C.c_uint8)), 6, 1 if compressed else 0, p32(out.view(np.uint32)))
    if not compressed:
        assert bad == 1


def test_pallas_square_root_tonelli_shanks_rejects_non_residues():
    """Compressed Pallas points go through Tonelli-Shanks (2-adicity 32): an x whose x^3 + 5 is not a square must be counted
    as invalid, both roots of a valid one must come back as flagged."""
    curve = "pallas"
    p = R.FIELDS["pallas_fq"]["p"]
    xs_bad = [x for x in range(2, 60) if pow((x ** 3 + 5) % p, (p - 1) // 2, p) == p - 1][:4]
    assert len(xs_bad) == 4
    body = b"".join(x.to_bytes(33, "little") for x in xs_bad)
    arr = np.frombuffer(body, dtype=np.uint8).copy()
    out = np.zeros((4, 8), dtype=np.uint64)
    assert emu().emu_srs_decode(2, arr.ctypes.data_as(C.POINTER(C.c_uint8)), 4, 1, p32(out.view(np.uint32))) == 4
    # a valid x with both flags
    x = next(x for x in range(2, 60) if pow((x ** 3 + 5) % p, (p - 1) // 2, p) == 1)
    for flag in (0, 0x80):
        b = bytearray(x.to_bytes(33, "little")); b[-1] |= flag
        arr = np.frombuffer(bytes(b), dtype=np.uint8).copy()
        out = np.zeros((1, 8), dtype=np.uint64)
        assert emu().emu_srs_decode(2, arr.ctypes.data_as(C.POINTER(C.c_uint8)), 1, 1, p32(out.view(np.uint32))) == 0
        (px, py), = O.array_to_points(curve, out)
        assert px == x and (py * py - x ** 3 - 5) % p == 0 and (py > p - py) == bool(flag)


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("curve", CURVES)
def test_msm_batch_over_key_table_stepped(curve, glv):
    """pc_hip_msm_batch's fast path: several polynomials of equal length in SEPARATE buffers go through one many-MSM
    pass over the key's own window table (bucket set k = polynomial k), here with fewer polynomials than bucket sets,
    a base offset and Montgomery scalars.  glv = 1: the key's table is the GLV one (two bucket sets per polynomial, phi on the
    second set's sum before the pair is added on the host)."""
    n_srs, off, m, B, count, c = 60, 7, 40, 4, 3, 6
    emu().emu_set_many_glv(glv)
    b = O.gen_bases(curve, n_srs)
    vecs = [O.gen_scalars(curve, 0x7A0 + k, m) for k in range(count)]
    mont = [O.f_to_mont(curve, 1, v) for v in vecs]
    arr = (C.c_void_p * count)(*[v.ctypes.data for v in mont])
    out = np.zeros((B, 2 * O.fq_limbs(curve)), dtype=np.uint64)
    emu().emu_msm_many_vectors(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(n_srs), C.c_size_t(off), C.c_size_t(m), arr, C.c_size_t(count),
                               C.c_size_t(B), c, 1, p32(out.view(np.uint32)))
    emu().emu_set_many_glv(0)
    for k in range(count):
        assert (out[k] == O.msm_naive(curve, np.ascontiguousarray(b[off:off + m]), vecs[k])).all(), k
    assert not out[count:].any()


@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_window_table_mul_stepped(curve):
    """`g.batch_mul(scalars)` (KZG10::setup, kzg10/mod.rs:76,83) with the fixed-base window table: signed radix-256
    digits, one mixed addition per window, XYZZ results normalised K at a time -- against Python big ints, including
    0, 1, r - 1 and scalars whose top window only receives the recoding carry."""
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    G = R.gen_bases(curve, 4)[3]
    ks = [0, 1, 2, 127, 128, 129, 255, 256, p - 1, p - 2, (1 << 200) - 1, 0x8080808080808080, (p >> 1) | 0xFF] + R.gen_scalars(fr, 0xF1, 9)
    ks = [k % p for k in ks]
    sc = O.fr_mont_array(curve, ks)
    g = O.points_to_array(curve, [G])[0]
    want = [R.ec_mul(curve, k, G) for k in ks]
    for K in (1, 5, 16):
        out = np.zeros((len(ks), 2 * O.fq_limbs(curve)), dtype=np.uint64)
        emu().emu_fixed_base_table(O.CURVES[curve], p32(g.view(np.uint32)), p32(sc.view(np.uint32)), C.c_size_t(len(ks)), K, p32(out.view(np.uint32)))
        assert O.array_to_points(curve, out) == want, K


@pytest.mark.parametrize("curve", CURVES)
def test_window_table_batched_build_equals_serial_build(curve):
    """pc_hip_srs_precompute's table: the window-by-window build with batched normalisation writes exactly what the
    one-lane-per-base build writes (incl. an infinity base and padded entries), for two window widths."""
    n = 11
    b = O.gen_bases(curve, n)
    b[4] = 0
    aw = b.shape[1] * 2
    for c, stride, K in ((13, aw, 4), (22, aw + 8, 16)):
        assert emu().emu_table_builds_agree(O.CURVES[curve], p32(b.view(np.uint32)), n, c, stride, K) == 1, (c, stride)


@pytest.mark.parametrize("curve", CURVES)
def test_msm_in_parts_stepped(curve):
    """MsmPlan::begin_parts / add_part (pc_hip_msm and pc_hip_kzg_open on host memory: ONE MSM in parts -- every part after the first
    accumulates into a second bucket array that BucketMergeBody folds into the first, one bucket reduction closes the call): the point
    of the undivided MSM for 1 .. 5 parts, with the window table (plain and GLV form) and table-free, a base offset, Montgomery input,
    buckets that only one part touches (sparse scalars) and buckets every part touches (five-valued scalars)."""
    n = 240
    b = O.gen_bases(curve, n)
    b[7] = 0
    uni = O.gen_scalars(curve, 23, n)
    few = np.ascontiguousarray(uni[np.arange(n) % 5])
    sparse = np.where((np.arange(n) % 9 == 0)[:, None], uni, 0).astype(np.uint64)

    def run(s, c, glv, parts, base_off=0, from_mont=0):
        out = np.zeros(2 * O.fq_limbs(curve), dtype=np.uint64)
        rc = emu().emu_msm_parts(O.CURVES[curve], p32(b.view(np.uint32)), C.c_size_t(len(b)), p32(s.view(np.uint32)), C.c_size_t(len(s)),
                                 base_off, c, glv, parts, from_mont, p32(out.view(np.uint32)))
        assert rc == 0
        return out
    for s in (uni, few, sparse):
        want = O.msm_naive(curve, b, s)
        for c, glv in ((7, 0), (9, 1), (0, 0)):
            for parts in (1, 2, 3, 5):
                assert (run(s, c, glv, parts) == want).all(), (c, glv, parts)
    part = np.ascontiguousarray(uni[:150])
    assert (run(part, 8, 0, 4, base_off=60) == O.msm_naive(curve, b[60:], part)).all()
    assert (run(O.f_to_mont(curve, 1, uni), 6, 1, 3, from_mont=1) == O.msm_naive(curve, b, uni)).all()
    assert not run(np.zeros((n, 4), dtype=np.uint64), 7, 0, 3).any()


# ---- the fold table of an IPA committer key in its general form (csrc/fold_table.hpp, glv.hpp) ----------------------------------------
@pytest.mark.parametrize("w", [2, 3, 4, 5])
def test_wnaf_digits(w):
    """Width-w NAF of 160-bit magnitudes: the digits rebuild the value, are odd and below 2^(w-1), and no two non-zero digits sit within
    w positions of each other (what bounds the additions per term at 130 / (w + 1))."""
    rnd = random.Random(w)
    vals = [0, 1, 2, 3, (1 << 130) - 1, 1 << 129, (1 << 128) + 1, 0xAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA] + [rnd.getrandbits(rnd.choice([8, 64, 128, 130])) for _ in range(200)]
    for v in vals:
        k = np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(5)], dtype=np.uint32)
        out = np.zeros(200, dtype=np.int8)
        ln = emu().emu_wnaf(p32(k), w, out.ctypes.data_as(C.POINTER(C.c_int8)))
        assert sum(int(d) << i for i, d in enumerate(out)) == v
        nz = [i for i, d in enumerate(out) if d]
        assert all(int(out[i]) % 2 and abs(int(out[i])) < (1 << (w - 1)) for i in nz)
        assert all(b - a >= w for a, b in zip(nz, nz[1:]))
        assert ln == (nz[-1] + 1 if nz else 0) and ln <= 131


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("levels,w", [(1, 2), (1, 4), (2, 2), (2, 3), (2, 4), (2, 5), (1, 5)])
def test_fold_table_one_and_two_levels(curve, levels, w):
    """Table build (affine doublings, odd multiples by affine additions) + the fold out of it, stepped on the CPU, against Python big
    ints: one level = K[i] + u1 K[h + i]; two levels = the key after the folds by u1 and by u2 (ipa_pc/mod.rs:699-707 twice), i.e.
    K[i] + u2 K[q + i] + u1 K[2q + i] + u1 u2 K[3q + i].  A point at infinity sits in every quarter of the key."""
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    n = 16
    pts = R.gen_bases(curve, n + 3)[3:]
    for j in (1, 6, 9, 15):
        pts[j] = None
    key = O.points_to_array(curve, pts)
    u1, u2 = R.gen_scalars(fr, 0xF01D + levels, 2)
    out = np.zeros((n >> levels, key.shape[1]), dtype=np.uint64)
    um = O.fr_mont_array(curve, [u1, u2])
    ok = emu().emu_fold_table(O.CURVES[curve], p32(key.view(np.uint32)), n, levels, w, p32(um[0].view(np.uint32)), p32(um[1].view(np.uint32)),
                              p32(out.view(np.uint32)))
    assert ok == 1
    got = O.array_to_points(curve, out)
    h = n // 2
    k1 = [R.ec_add(curve, pts[i], R.ec_mul(curve, u1, pts[h + i])) for i in range(h)]
    if levels == 1:
        assert got == k1
    else:
        q = n // 4
        assert got == [R.ec_add(curve, k1[i], R.ec_mul(curve, u2, k1[q + i])) for i in range(q)]


# ---- sums that become the point at infinity inside the pipeline (tests/harness/signedkey.py; the device runs tests/test_msm_cancel_gpu.py) ----
def _cancel_rows(curve, m, start, seed):
    """[random, const (cancels), copy of row 0, all_but_one] against key positions start .. start + m of signed(.., holes=True)"""
    from harness import signedkey as SK
    lay = SK.layouts(curve, m, seed, start, holes=True)
    rnd = SK.rand_scalars(curve, m, seed + 1)
    return [rnd, lay["const"], list(rnd), lay["all_but_one"]]


@pytest.mark.parametrize("curve", CURVES)
def test_many_mode_stepped_rows_that_cancel_beside_rows_that_do_not(curve):
    """Many-MSM mode, m = 40, B = 4, c = 6, on a key of P, -P neighbours with a hole: bucket set 1 holds nothing but sums that cancelled
    (its row is the point at infinity, all-zero words), between sets 0 and 2 that hold the same finite sums, and set 3 one entry off
    a cancelling row.  pc_hip_msm_many's form (one scalar matrix, the pass's own table) and the batch fast path's (separate vectors
    over the key's table from an odd offset, plain and GLV form, fewer vectors than bucket sets); then ONE base under one scalar per
    row, where every join of a row adds equal sums.  Expected: Python integers and one scalar multiplication."""
    from harness import signedkey as SK
    m, B, c = 40, 4, 6
    nq = 2 * O.fq_limbs(curve)
    key = SK.signed(curve, m, holes=True)
    rows = _cancel_rows(curve, m, 0, 0xE40)
    want = np.stack([SK.expected(key, r) for r in rows])
    assert not want[1].any() and want[0].any() and want[3].any() and (want[0] == want[2]).all()
    flat = SK.limbs([v for r in rows for v in r])
    for K0 in (2, 0, 4):
        out = np.ones((B, nq), dtype=np.uint64)
        emu().emu_msm_many(O.CURVES[curve], p32(key.bases.view(np.uint32)), C.c_size_t(m), p32(flat.view(np.uint32)), C.c_size_t(B), c, K0, 0, p32(out.view(np.uint32)))
        assert (out == want).all(), K0
    one = SK.one_base(curve, m)
    ks = [1, 3, SK.rand_scalars(curve, 1, 7)[0], 0]
    eq = [[k] * m for k in ks]
    out = np.ones((B, nq), dtype=np.uint64)
    emu().emu_msm_many(O.CURVES[curve], p32(one.bases.view(np.uint32)), C.c_size_t(m), p32(SK.limbs([v for r in eq for v in r]).view(np.uint32)), C.c_size_t(B), c, 2, 0,
                       p32(out.view(np.uint32)))
    assert (out == np.stack([SK.expected(one, r) for r in eq])).all()
    # separate vectors, the key's own table, base offset 7 (odd: the layouts are laid against positions 7 .. 47)
    off = 7
    big = SK.signed(curve, m + off, holes=True)
    rows = _cancel_rows(curve, m, off, 0xE41)
    want = np.stack([SK.expected(big, r, off) for r in rows])
    assert not want[1].any() and want[3].any()
    # (the chunk length of a batch pass is the key's: the context's tuning at upload; 1, 2 and 5 entries per lane as the device test sets them)
    for glv, T in ((0, 0), (1, 0), (0, 1), (0, 2), (1, 5), (0, 5)):
        for vecs in (rows, rows[1:3]):                                           # four vectors in four sets; two in four: the cancelling row first
            mont = [SK.mont(curve, r) for r in vecs]
            arr = (C.c_void_p * len(vecs))(*[v.ctypes.data for v in mont])
            out = np.ones((B, nq), dtype=np.uint64)
            emu().emu_set_many_glv(glv)
            emu().emu_set_many_chunk(T)
            try:
                emu().emu_msm_many_vectors(O.CURVES[curve], p32(big.bases.view(np.uint32)), C.c_size_t(m + off), C.c_size_t(off), C.c_size_t(m), arr,
                                           C.c_size_t(len(vecs)), C.c_size_t(B), c, 1, p32(out.view(np.uint32)))
            finally:
                emu().emu_set_many_glv(0)
                emu().emu_set_many_chunk(0)
            w = want if len(vecs) == 4 else want[1:3]
            assert (out[:len(vecs)] == w).all(), (glv, T, len(vecs))
            assert not out[len(vecs):].any()


@pytest.mark.parametrize("curve", CURVES)
def test_single_msm_stepped_on_cancelling_layouts(curve):
    """The single MSM's stepped entries on the same key: table-free under chunks of 1, 2, 5 and 8 entries (an even chunk's partial sum
    is the point at infinity and is written to its slot as such; odd chunks alternate +-k P and cancel in the joins), the window table
    in its plain and GLV form (both halves of a pair's scalar split alike: both bucket sets cancel), and the MSM in parts on the
    halves key, where every bucket of the later parts is the negative of the first part's and BucketMergeBody adds P and -P."""
    from harness import signedkey as SK
    n = 64
    key = SK.signed(curve, n, holes=True)
    lay = SK.layouts(curve, n, 0xE42, 0, holes=True)
    for name in ("const", "pairwise", "pairwise_few", "all_but_one"):
        s = SK.limbs(lay[name])
        want = SK.expected(key, lay[name])
        assert want.any() == (name == "all_but_one")
        for (c, T, T2, K0) in ((4, 1, 4, 2), (6, 2, 4, 2), (5, 5, 5, 2), (7, 8, 4, 4), (0, 0, 0, 0)):
            assert (run_msm(curve, key.bases, s, c, T, T2, K0) == want).all(), (name, c, T)
        for c, K0 in ((4, 2), (7, 0)):
            assert (run_msm_table(curve, key.bases, s, c, K0) == want).all(), (name, "table", c)
            assert (run_msm_table_glv(curve, key.bases, s, c, K0) == want).all(), (name, "glv table", c)
    un = SK.unsigned(curve, n)
    opp = SK.layouts(curve, n, 0xE43)["opposite_scalars"]
    assert not SK.expected(un, opp).any()
    assert not run_msm(curve, un.bases, SK.limbs(opp), 5, 5, 4, 2).any()
    # in parts: s[j] = s[j + n / 2] on halves(n)
    n = 240
    h = SK.halves(curve, n)
    half = SK.rand_scalars(curve, n // 2, 0xE44)
    one_off = half + half
    one_off[n // 2 + 17] = (one_off[17] + 5) % SK.modulus(curve)
    for s in (half + half, one_off):
        want = SK.expected(h, s)
        assert want.any() == (s is one_off)
        for c, glv in ((7, 0), (9, 1), (0, 0)):
            for parts in (2, 4):
                out = np.ones(2 * O.fq_limbs(curve), dtype=np.uint64)
                assert emu().emu_msm_parts(O.CURVES[curve], p32(h.bases.view(np.uint32)), C.c_size_t(n), p32(SK.limbs(s).view(np.uint32)), C.c_size_t(n), 0, c, glv,
                                           parts, 0, p32(out.view(np.uint32))) == 0
                assert (out == want).all(), (c, glv, parts)
