"""The reference of the bucket sort's contract (tests/harness/sortref.py) checked on the CPU: the vectorised recoding against the
Python-integer one on the edge scalars, the three checks of check_sort against outputs that break them, and the reference's buckets
against the CPU-stepped atomic sort of tests/emu (sort_entries_atomic run lane by lane) in the plain, table, many-MSM and GLV modes.
The GPU file tests/test_msm_sort_gpu.py runs the same checks on the device sorts."""
import ctypes as C
import random

import numpy as np
import pytest

from harness import sortref as S
from test_emu_cpu import emu, p32

CURVES = list(S.CURVES)


def scalars_for(curve, c, n_rand, seed, glv=False):
    rnd = random.Random(seed)
    r = S.modulus(curve)
    return S.edge_scalars(curve, c, glv) + [rnd.randrange(r) for _ in range(n_rand)]


@pytest.mark.parametrize("curve", CURVES)
def test_vectorised_recoding_equals_integer_recoding_on_edge_scalars(curve):
    """recode() over the numpy limbs against recode_int() over Python integers: digit for digit, on the edge scalars of every width,
    over the scalar's windows and over the 130-bit halves' windows; every digit inside [-(2^(c-1) - 1), 2^(c-1)]"""
    bits = S.FR_BITS[curve]
    for c in range(2, 25):
        vals = scalars_for(curve, c, 20, c)
        windows = bits // c + 1
        d = S.recode(S.to_limbs(vals), c, windows)
        assert d.min() >= -((1 << (c - 1)) - 1) and d.max() <= 1 << (c - 1)
        for k, row in zip(vals, d):
            want = S.recode_int(k, c, windows)
            assert list(row) == want, (c, hex(k))
            assert sum(v << (c * w) for w, v in enumerate(want)) == k
        hw = S.HALF_BITS // c + 1
        hv = [v & ((1 << S.HALF_BITS) - 1) for v in vals]
        dh = S.recode(S.to_limbs(hv, S.HALF_WORDS), c, hw)
        for k, row in zip(hv, dh):
            assert list(row) == S.recode_int(k, c, hw), (c, hex(k))


def test_edge_scalars_hold_the_cases_they_promise():
    """the all-2^(c-1) scalar recodes without a carry into last buckets only; the all-(2^(c-1) + 1) one carries through every window
    into the top one; a scalar below the top window leaves it empty"""
    for curve in CURVES:
        bits, r = S.FR_BITS[curve], S.modulus(curve)
        for c in (3, 5, 11, 16, 17, 19, 23):
            windows, half = bits // c + 1, 1 << (c - 1)
            a = S.recode_int(S.pattern(half, c, bits, r), c, windows)
            assert set(a) <= {half, 0} and a.count(half) >= windows - 2
            b = S.recode_int(S.pattern(half + 1, c, bits, r), c, windows)
            k = max(w for w, v in enumerate(b) if v)
            assert b[0] == -(half - 1) and all(v == -(half - 2) for v in b[1:k]) and b[k] == 1 and k >= windows - 2
            assert S.recode_int((1 << (c * (bits // c))) - 1, c, windows)[-1] in (0, 1)
    # where c divides the width the top window has no scalar bits at all and holds the carry alone
    assert S.FR_BITS["bls12_381"] % 17 == 0 and S.FR_BITS["bls12_377"] % 23 == 0 and S.FR_BITS["bls12_377"] % 11 == 0
    top = S.recode_int(S.modulus("bls12_381") - 1, 17, 16)
    assert top[-1] == 1 and top[-2] < 0


def run_emu_sort(g, canon, from_mont=0):
    offsets = np.full(g.NB + 1, 0xffffffff, dtype=np.uint32)
    entries = np.full(g.n * g.Wd, 0xffffffff, dtype=np.uint32)
    sc = canon
    if from_mont:
        rmod = S.modulus(g.curve)
        sc = S.to_limbs([k * (1 << 256) % rmod for k in S.to_ints(canon)])
    rc = emu().emu_sort_atomic(S.CURVES[g.curve], C.c_size_t(g.n), g.c, g.tbl_stride, g.m_sub, g.glv, from_mont, g.base_off, p32(sc), p32(offsets), p32(entries))
    assert rc == 0
    return offsets, entries


MODES = ["plain", "table", "many", "glv", "many_glv"]


def geom_for(mode, curve, n, c, base_off=0):
    if mode == "plain":
        return S.Geom(curve, n, c, base_off=base_off)
    m = 7 if mode.startswith("many") else 0
    n = n - n % 7 if m else n
    return S.Geom(curve, n, c, tbl_stride=(m or n) + base_off + 3, m_sub=m, glv=int(mode.endswith("glv")), base_off=base_off)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("curve", CURVES)
def test_reference_buckets_equal_the_stepped_atomic_sort(curve, mode):
    """sort_entries_atomic stepped on the CPU against the reference, all three checks, in every mode: edge scalars and random ones,
    canonical and Montgomery input, a non-zero base offset"""
    for c, base_off, from_mont in ((3, 0, 0), (8, 5, 1), (13, 0, 0), (17, 1000, 0), (23 if curve == "bls12_377" and not mode.startswith("many") else 16, 0, 1)):
        vals = scalars_for(curve, c, 64, 100 + c, glv=mode.endswith("glv"))
        g = geom_for(mode, curve, len(vals), c, base_off)
        canon = S.to_limbs(vals[:g.n])
        offsets, entries = run_emu_sort(g, canon, from_mont)
        assert S.check_sort(g, canon, offsets, entries) > 0
        if not g.glv:
            rk, re = S.ref_sort(g, canon)
            assert sorted(zip(rk.tolist(), re.tolist())) == S.ref_sort_int(g, vals[:g.n])


def test_host_build_of_the_probe_has_the_sort_entry_points():
    """the sort is device code: the host build of tests/hip/probe_sort.hip compiles and answers PROBE_UNSUPPORTED, and PROBE_BAD_OP for
    a curve it does not know"""
    from harness import probe as P
    host, out = P.host_probe(), np.zeros(16, dtype=np.uint32)
    u = C.c_uint32
    assert host.raw("pc_probe_sort_geom", 1, C.c_size_t(5000), u(19), u(14), u(14), u(0), u(0), u(0), P.p32(out)) == P.UNSUPPORTED
    assert host.raw("pc_probe_sort_geom", 4, C.c_size_t(5000), u(19), u(14), u(14), u(0), u(0), u(0), P.p32(out)) == -2
    sc, path = np.zeros((1, 8), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert host.raw("pc_probe_sort", 1, C.c_size_t(1), u(19), u(14), u(14), u(0), u(0), u(0), u(0), u(0), 0, 0, P.p32(sc), P.p32(out), P.p32(out),
                    P.p32(path)) == P.UNSUPPORTED
    assert not out.any()


def test_checks_catch_a_wrong_sort():
    """check_sort fails on outputs that break one property each: an entry in the neighbouring bucket, a flipped sign, a digit dropped,
    a digit doubled, an entry swapped between two scalars of one bucket set"""
    rnd = random.Random(9)
    r = S.modulus("bn254")
    vals = [rnd.randrange(r) for _ in range(300)]
    for g in (S.Geom("bn254", 300, 5), S.Geom("bn254", 300, 9, tbl_stride=300), S.Geom("bn254", 300, 9, tbl_stride=300, glv=1)):
        canon = S.to_limbs(vals)
        offsets, entries = run_emu_sort(g, canon)
        M = S.check_sort(g, canon, offsets, entries)
        k = next(k for k in range(1, g.NB) if offsets[k] < offsets[k + 1])      # a non-empty bucket

        def broken(f):
            o, e = offsets.copy(), entries.copy()
            f(o, e)
            with pytest.raises(AssertionError):
                S.check_sort(g, canon, o, e)

        def move_boundary(o, e): o[k] += 1                                       # the bucket's first entry now belongs to bucket k - 1
        def flip_sign(o, e): e[o[k]] ^= 0x80000000
        def drop_last(o, e): o[-1] -= 1; e[M - 1] = 0xffffffff
        def other_scalar(o, e): e[o[k]] ^= 1
        def write_behind(o, e): e[M] = 0
        for f in (move_boundary, flip_sign, drop_last, other_scalar, write_behind):
            broken(f)
