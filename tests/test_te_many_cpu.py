"""CPU-only checks of the many-MSM pass over a twisted Edwards key (csrc/te.hpp: TeWindowRowBody and te_window_table; csrc/msm.hpp:
MsmPlan<TeOf<ed_on_bls12_381>> with a bucket set per sub-MSM, SubFoldBody, one normalisation for all results), compiled for the host
by tests/emu/emu_te_many.cpp and stepped lane by lane, against the pure-Python restatement tests/harness/teref.py.  Every comparison
is bit-exact on the affine Montgomery bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from harness import teref as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_te_many.so")
        srcs = [os.path.join(HERE, "emu", "emu_te_many.cpp")] + [
            os.path.join(ROOT, "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "msm_sort.hpp", "ec.hpp", "fp32.hpp", "te.hpp", "te_constants.h", "host_tail.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        _emu.emu_te_msm_many.restype = C.c_int
        _emu.emu_te_plan_refuses.restype = C.c_int
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def resident(pts):
    return np.concatenate([E.resident_words(p) for p in pts])


def from_resident(words):
    """(x, y) of a 24-word resident point, with its third coordinate checked: td = 2 d x y"""
    p = E.point_from_bytes(words[:16].tobytes())
    assert (words == E.resident_words(p)).all(), "the derived coordinate is not 2 d x y"
    return p


def shape(m):
    c, Wd = C.c_uint32(0), C.c_uint32(0)
    emu().emu_te_many_shape(C.c_size_t(m), C.byref(c), C.byref(Wd))
    return c.value, Wd.value


@pytest.fixture(scope="module")
def key40():
    ks = [(i * 0x9e3779b97f4a7c15 + 777) ** 3 % E.R for i in range(40)]
    return E.fixed_base(E.GEN).mul_many(ks)


def test_shape_is_the_librarys_choice():
    """c and the row count of the table come from msm_choose_table_c(m, 252, 0) and msm_num_windows: every digit of a 252-bit scalar,
    the carry of the signed recoding included, has a row"""
    for m in (1, 2, 5, 33, 65, 1025):
        c, Wd = shape(m)
        assert 8 <= c <= 23 and Wd == 252 // c + 1 and c * Wd > 252


@pytest.mark.parametrize("c,Wd,K", [(8, 32, 16), (5, 51, 3), (13, 20, 1)])
def test_window_table_rows(key40, c, Wd, K):
    """T[w][j] = 2^(c w) P_j for points of order 2, 4 and 8, the identity, the all-zero entry, P beside -P and points outside the
    prime-order subgroup: the doubling is exact on whatever it is given (2^(c w) is NOT reduced modulo r), and the lanes of one
    inversion group (K points, the last group partial) do not disturb each other.  The all-zero entry stays all zero in row 0 and is
    the identity in every later row."""
    P = key40[0]
    bases = [E.T2, E.T4, E.T8, E.IDENT, E.ZERO, P, E.neg(P), E.add(key40[1], E.T8), E.add(key40[2], E.T4)] + list(key40[3:8])
    m = len(bases)
    table = np.zeros(Wd * m * 24, dtype=np.uint32)
    emu().emu_te_window_table(p32(resident(bases)), C.c_size_t(m), c, Wd, K, p32(table))
    for j, b in enumerate(bases):
        want = b
        for w in range(Wd):
            rec = table[(w * m + j) * 24:(w * m + j + 1) * 24]
            if b == E.ZERO:
                assert (not rec.any()) if w == 0 else from_resident(rec) == E.IDENT, (j, w)
            else:
                assert from_resident(rec) == want, (j, w)
                for _ in range(c):
                    want = E.add(want, want)
    # what the rows of P and -P hold: negations of each other, (-x, y, -td)
    for w in range(Wd):
        a, b = table[(w * m + 5) * 24:(w * m + 6) * 24], table[(w * m + 6) * 24:(w * m + 7) * 24]
        assert E.neg(from_resident(a)) == from_resident(b)


def run_many(bases, rows, m, base_off=0, c=0, T=0, T2=0, K0=0, mont=False, empty=False):
    B = len(rows)
    s = E.scalars_array([k for r in rows for k in r], mont).view(np.uint32)
    out = np.zeros(16 * B, dtype=np.uint32)
    rc = emu().emu_te_msm_many(p32(resident(bases)), base_off, C.c_size_t(m), p32(s), C.c_size_t(B), c, T, T2, K0, int(mont), int(empty), p32(out))
    assert rc == 0
    return [out[16 * k:16 * k + 16].tobytes() for k in range(B)]


def many_bases(key, m):
    """the first m of: subgroup points with the low-order points, the identity, the all-zero entry and P beside -P among them"""
    b = list(key)
    if m >= 5:
        b[1], b[2] = E.T8, E.ZERO
        b[4] = E.neg(b[3])
    if m >= 33:
        b[7], b[8], b[9] = E.T2, E.T4, E.IDENT
        b[12] = b[11]
        for i in range(20, 30):
            b[i] = E.add(b[i], E.T8)
    return b[:m]


def many_rows(m, B, seed):
    """B rows of m scalars: random ones with 0, 1, r - 1 and 2^251 mixed in; row 1 (if any) all zero; the last row of a pass with
    m >= 5 cancels to the identity: k P + k (-P)"""
    rnd = np.random.RandomState(seed)
    special = [0, 1, E.R - 1, 1 << 251]
    rows = []
    for k in range(B):
        row = [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(m)]
        for j in range(m):
            if (j + k) % 3 == 0:
                row[j] = special[(j + 2 * k) % 4]
        rows.append(row)
    if B > 1:
        rows[1] = [0] * m
    if m >= 5 and B > 2:
        rows[-1] = [0] * m
        rows[-1][3] = rows[-1][4] = 0x123456789abcdef123456789
    return rows


SETTINGS = ((0, 0, 0, 0), (5, 4, 4, 2), (9, 7, 5, 4))      # (c, T, T2, K0); c = 0: the library's width


@pytest.mark.parametrize("m,B", [(1, 1), (2, 3), (5, 4), (33, 8)])
def test_te_msm_many_stepped(key40, m, B):
    """Every row of a many-MSM pass equals teref.msm of that row, at the library's width and at two others with short chunks (buckets
    cut across lanes, serial and cooperative reduction levels); an all-zero row and a row that cancels are the identity (0, ONE),
    never zeros; both scalar forms; a base offset."""
    bases = many_bases(key40, m)
    rows = many_rows(m, B, 100 * m + B)
    want = [E.point_bytes(E.msm(bases, r)) for r in rows]
    if B > 1:
        assert want[1] == E.IDENT_BYTES
    if m >= 5 and B > 2:
        assert want[-1] == E.IDENT_BYTES
    for (c, T, T2, K0) in SETTINGS:
        assert run_many(bases, rows, m, 0, c, T, T2, K0) == want, (c, T, T2, K0)
    assert run_many(bases, rows, m, mont=True) == want
    # the same rows against the same points at an offset inside a longer key
    longer = [E.T4, key40[39], E.ZERO] + bases + [key40[38]]
    assert run_many(longer, rows, m, base_off=3) == want


def test_te_msm_many_all_rows_without_a_digit(key40):
    """No non-zero digit anywhere (every bucket set stays empty), and a call with no pairs at all (MsmPlan's pending_empty_ path):
    B identities (0, ONE)"""
    bases = many_bases(key40, 5)
    rows = [[0] * 5 for _ in range(3)]
    assert run_many(bases, rows, 5) == [E.IDENT_BYTES] * 3
    assert run_many(bases, rows, 5, empty=True) == [E.IDENT_BYTES] * 3


def test_plan_still_refuses_a_single_msm_table():
    """A twisted Edwards single-MSM plan handed a window table is refused as before; so is the many-MSM mode without a table."""
    assert emu().emu_te_plan_refuses(0) == 1
    assert emu().emu_te_plan_refuses(1) == 1
