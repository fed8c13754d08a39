"""CPU suite for the radix-2^30 form of BLS12-381 Fq (csrc/fp30.hpp) and the running sum built on it (csrc/ec.hpp XyzzR30):
every field operation against Python integers, on the boundary values of each operand class and on random ones, every output
against the class its function states; the conversions from and to the 12-word Montgomery layout; the compile-time column plan
re-checked with independent worst-case bounds; chains of mixed additions against XyzzD::add_affine_lz; and the same chains once
under AddressSanitizer + UBSan (a program of its own: tests/emu/emu_fq30.cpp with FQ30_SELFTEST_MAIN)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pyref as R

from harness.fq30ref import MASK, N, P, R32, RP, W, class_values, from12, from13, mont, mul_out, normalised, to12, to13

HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = [os.path.join(HERE, "emu", "emu_fq30.cpp")] + [os.path.join(HERE, "..", "poly_commit_amd", "csrc", f) for f in ("fp30.hpp", "fp32.hpp", "ec.hpp")]
_libs = {}
_form = "rows"


@pytest.fixture(params=["rows", "columns"], autouse=True)
def form(request):
    """every test runs on both host forms of the multiplier: by rows (what the CPU-stepped kernels use) and by columns -- the
    device's own product-scanning code with its set-aside splits, the multiply-adds as wrapping 64-bit arithmetic
    (PC_FQ30_HOST_COLUMNS)"""
    global _form
    _form = request.param
    yield
    _form = "rows"


def _flags():
    return ["-DPC_FQ30_HOST_COLUMNS"] if _form == "columns" else []


def lib():
    if _form not in _libs:
        so = os.path.join(HERE, "emu", "libemu_fq30_%s.so" % _form)
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in _SRC):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *_flags(), "-o", tmp, _SRC[0]])
            os.replace(tmp, so)
        _libs[_form] = C.CDLL(so)
    return _libs[_form]


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def op(code, *args, n_out=13):
    ins = [a if isinstance(a, np.ndarray) else to13(a) for a in args]
    while len(ins) < 4:
        ins.append(np.zeros(13, dtype=np.uint32))
    out = np.zeros(13, dtype=np.uint32)
    assert lib().fq30_op(code, p32(ins[0]), p32(ins[1]), p32(ins[2]), p32(ins[3]), p32(out)) == 0
    return out[:n_out]


def test_constants():
    assert RP // P >= 630                                      # the rule behind mul_out
    assert from13(op(10)) == RP % P                            # one()
    assert from13(op(6, to12(R32 % P))) == 64 * (R32 % P)


@pytest.mark.parametrize("code,VA,VB", [(0, 64, 2), (13, 66, 8)])
def test_mul(code, VA, VB):
    rnd = random.Random(30 + code)
    for a in class_values(VA, rnd):
        for b in class_values(VB, rnd):
            got = op(code, a, b)
            assert normalised(got)
            assert from13(got) == mont(a * b), (a, b)
            assert from13(got) <= mul_out(VA * VB) * P


def test_mul_stated_bound_of_the_load():
    """a table operand (below 64p) times a product output (below 2p) stays below 1.21 p"""
    rnd = random.Random(5)
    worst = 0
    for a in class_values(64, rnd, 40):
        for b in class_values(2, rnd, 6):
            worst = max(worst, from13(op(0, a, b)))
    assert worst * 100 < 121 * P


def test_sqr():
    rnd = random.Random(31)
    for a in class_values(66, rnd, 60):
        got = op(1, a)
        assert normalised(got)
        assert from13(got) == mont(a * a), a
        assert from13(got) <= mul_out(66 * 66) * P


def test_mul_add_mul():
    rnd = random.Random(32)
    A, B, Cc, D = (class_values(v, rnd, 4) for v in (66, 16, 64, 2))
    worst = (66 * P, 16 * P, 64 * P, 2 * P)
    cases = [worst] + [(rnd.choice(A), rnd.choice(B), rnd.choice(Cc), rnd.choice(D)) for _ in range(400)]
    for a, b, c, d in cases:
        got = op(2, a, b, c, d)
        assert normalised(got)
        assert from13(got) == mont(a * b + c * d), (a, b, c, d)
        assert from13(got) <= mul_out(66 * 16 + 64 * 2) * P


@pytest.mark.parametrize("code,VA,V,factor", [(3, 2, 64, 1), (11, 8, 2, 1), (12, 2, 14, 1), (4, 10, 4, 2)])
def test_sub(code, VA, V, factor):
    """sub<V>(a, b) = a - b + V p for b <= V p; sub_dbl<V>(a, b) = a - 2b + V p for 2b <= V p: exact integers, normalised limbs, class VA + V"""
    rnd = random.Random(33 + code)
    for a in class_values(VA, rnd):
        for b in class_values(V // factor, rnd):
            got = op(code, a, b)
            assert normalised(got)
            assert from13(got) == a - factor * b + V * P, (a, b)
            assert from13(got) <= (VA + V) * P


def test_neg():
    rnd = random.Random(34)
    for a in class_values(64, rnd, 60):
        got = op(5, a)
        assert normalised(got)
        assert from13(got) == 64 * P - a


def test_conversions():
    """from32: a 12-word residue w <= p becomes 64 w (the same residue for R' = 2^390, below or at 64p); to32: back to R = 2^384 form
    below 2p; the two are inverse modulo p and agree with the 32-bit Montgomery form x 2^384 <-> x 2^390"""
    rnd = random.Random(35)
    for w in [0, 1, 2, P - 2, P - 1, P, R32 % P] + [rnd.randrange(P) for _ in range(200)]:
        a = op(6, to12(w))
        assert normalised(a) and from13(a) == 64 * w
        back = op(7, a, n_out=12)
        assert from12(back) < 2 * P and from12(back) % P == w % P
        x = w * pow(R32, -1, P) % P                            # the element w stands for
        assert from13(a) % P == x * RP % P
    # to32 on any class-64 value, and the exact zero that marks infinity
    for v in class_values(64, rnd, 100):
        back = from12(op(7, v, n_out=12))
        assert back < 2 * P and back % P == v * R32 * pow(RP, -1, P) % P
    assert from12(op(7, 0, n_out=12)) == 0
    # reduce(): class 64 -> class 2, same residue
    for v in class_values(64, rnd, 50):
        r = op(9, v)
        assert normalised(r) and from13(r) <= 2 * P and from13(r) % P == v % P


def test_is_zero():
    rnd = random.Random(36)
    for k in range(67):
        assert op(8, k * P, n_out=1)[0] == 1
        if k:
            assert op(8, k * P - 1, n_out=1)[0] == 0
        if k < 66:
            assert op(8, k * P + 1, n_out=1)[0] == 0
            assert op(8, k * P + (1 << 30) * rnd.randrange(1, 1 << 200), n_out=1)[0] == 0      # limb 0 of k p, another value
    for _ in range(300):
        v = rnd.randrange(66 * P)
        assert op(8, v, n_out=1)[0] == (1 if v % P == 0 else 0)
    assert op(14, 0, n_out=1)[0] == 1 and op(14, P, n_out=1)[0] == 0 and op(14, 1 << 360, n_out=1)[0] == 0


@pytest.mark.parametrize("kind,V", [(0, (64, 2, 0, 0)), (0, (66, 8, 0, 0)), (0, (64, 8, 0, 0)), (0, (2, 8, 0, 0)), (0, (2, 2, 0, 0)), (0, (64, 1, 0, 0)),
                                    (1, (66, 66, 0, 0)), (2, (66, 16, 64, 2))])
def test_column_plan(kind, V):
    """The compile-time plan (which columns move the accumulator's high word aside, and before which group of terms), replayed
    here with independently computed worst cases: limbs 0..11 at 2^30 - 1, limb 12 at the class's top, every m_i at 2^30 - 1, the
    limbs of p as they are.  No partial sum may pass 2^64 - 1, nor the carry into the next column."""
    split = np.zeros(75, dtype=np.uint8)
    ok = lib().fq30_plan(kind, *V, split.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert ok == 1
    pl = [(P >> (W * i)) & MASK for i in range(13)]

    def lmax(v, i):
        return MASK if i < 12 else (v * P) >> 360

    carry, cols = 0, []
    for k in range(25):
        i0, i1 = max(0, k - 12), min(12, k)
        g = [0, 0, 0]
        for i in range(i0, i1 + 1):
            j = k - i
            if kind == 1:
                g[0] += lmax(V[0], i) * 2 * lmax(V[0], j) if i < j else (lmax(V[0], i) ** 2 if i == j else 0)
            else:
                g[0] += lmax(V[0], i) * lmax(V[1], j)
                g[1] += lmax(V[2], i) * lmax(V[3], j) if kind == 2 else 0
            g[2] += MASK * pl[j]
        acc, aside = carry, 0
        for gi in range(3):
            if split[3 * k + gi]:
                aside += acc >> 32
                acc &= 0xffffffff
                cols.append(k)
            acc += g[gi]
            assert acc < 1 << 64, (k, gi)
        carry = (acc >> 30) + (aside << 2)
        assert carry < 1 << 64 and aside < 1 << 64
    assert carry < 1 << 32
    print("plan", kind, V, "columns with a split:", sorted(set(cols)))


def _chain(idx):
    idx = np.asarray(idx, dtype=np.uint32)
    o30, olz, oc = (np.zeros(48, dtype=np.uint32) for _ in range(3))
    bad = lib().fq30_chain(C.c_size_t(len(idx)), p32(idx), p32(o30), p32(olz), p32(oc))
    return bad, o30, olz, oc


def _affine(xyzz):
    """(x, y) of a canonical XYZZ point in the 12-word Montgomery layout, or None for infinity"""
    X, Y, ZZ, ZZZ = (from12(xyzz[12 * i:12 * i + 12]) for i in range(4))
    if ZZ == 0:
        return None
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


NEG = 1 << 31


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_add_affine_random_chain(seed):
    """1500 additions of random table points (entry 0: the infinite base; signed digits), the radix-2^30 sum compared with
    add_affine_lz after EVERY step (canonicalised) together with its class invariant, and with the canonical addition at the end"""
    rnd = random.Random(seed)
    idx = [rnd.randrange(64) | (NEG if rnd.random() < 0.5 else 0) for _ in range(1500)]
    bad, o30, olz, oc = _chain(idx)
    assert bad == 0
    assert (o30 == olz).all()
    assert _affine(o30) == _affine(oc)


def test_add_affine_special_cases():
    cases = {
        "infinite sum, infinite base": [0, 0],
        "infinite base on a finite sum": [3, 0, 0 | NEG, 4],
        "doubling": [5, 5, 7],
        "doubling of a negated digit": [5 | NEG, 5 | NEG, 9],
        "P + (-P), then on from infinity": [6, 6 | NEG, 2, 3],
        "(-P) + P": [6 | NEG, 6, 2 | NEG],
        "doubling deeper in a chain": [1, 2, 3, 6, 12, 24, 48],            # 1 + 2 = 3: + 3 doubles, + 6 doubles, ...
        "cancelling deeper in a chain": [1, 2, 3 | NEG, 5, 5],
        "negated digit": [9 | NEG, 4, 17 | NEG],
    }
    for name, idx in cases.items():
        bad, o30, olz, oc = _chain(idx)
        assert bad == 0, name
        assert (o30 == olz).all() or (_affine(o30) is None and _affine(olz) is None), name
        assert _affine(o30) == _affine(oc), name
    assert _affine(_chain(cases["P + (-P), then on from infinity"][:2])[1]) is None


def test_selftest_under_sanitizers(tmp_path):
    """the chains of emu_fq30.cpp's own main() (4000 additions with the special cases) under AddressSanitizer + UBSan"""
    exe = str(tmp_path / "fq30_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-std=c++17",
                           *_flags(), "-DFQ30_SELFTEST_MAIN", "-o", exe, _SRC[0]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 bad steps, affine sums equal" in r.stdout
