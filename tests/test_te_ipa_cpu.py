"""CPU-only checks of the device path of InnerProductArgPC over ed_on_bls12_381: the new bodies of csrc/te.hpp (fold table rows, table
fold, out-of-place fold, subgroup check) and the functor bodies of csrc/ipa.hpp instantiated for the curve's 252-bit scalar field,
compiled for the host by tests/emu/emu_te_ipa.cpp and stepped lane by lane, against the pure-Python restatement
tests/harness/te_ipa.py; bit-exact on the Montgomery bytes.  Then what needs no device of the built library and the Python side: the
argument checks of every new entry point, and the transcript's byte conventions against hand-computed bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from harness import te_ipa as H
from harness import teref as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_te_ipa.so")
        srcs = [os.path.join(HERE, "emu", "emu_te_ipa.cpp")] + [
            os.path.join(ROOT, "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "ipa.hpp", "ec.hpp", "fp32.hpp", "te.hpp", "te_constants.h", "host_tail.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        _emu.emu_te_ipa_fold_from.restype = C.c_int
    return _emu


def p32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def resident(pts):
    return np.concatenate([E.resident_words(p) for p in pts])


def from_resident(words):
    p = E.point_from_bytes(words[:16].tobytes())
    assert (words == E.resident_words(p)).all(), "the derived coordinate is not 2 d x y"
    return p


def fr_words(ks):
    return E.scalars_array(ks, True).view(np.uint32).reshape(-1).copy()


def fr_ints(words):
    ri = pow(E.MONT_R, -1, E.R)
    out = []
    for i in range(len(words) // 8):
        v = int.from_bytes(words[8 * i:8 * i + 8].tobytes(), "little")
        assert v < E.R, "a scalar left [0, r)"
        out.append(v * ri % E.R)
    return out


def rand_scalars(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


U_SET = [0, 1, 2, E.R - 1, E.R - 2, int("55" * 31, 16) % E.R, 1 << 251, rand_scalars(7, 1)[0]]


# ---- Fr bodies ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_emu_fr_powers(n):
    for z in (0, 1, E.R - 1, rand_scalars(n, 1)[0]):
        out = np.zeros(8 * n, dtype=np.uint32)
        emu().emu_te_ipa_fr_powers(p32(fr_words([z])), C.c_size_t(n), p32(out))
        assert fr_ints(out) == H.powers(z, n), z


def test_emu_key_scalars_down_to_the_last_fold():
    """n0 = 64: the rounds at m = 64 .. 2 with the fold of the round before applied first, then the final fold of size 2"""
    n0 = 64
    c = rand_scalars(1, n0)
    s_want = [1] * n0
    s = fr_words(s_want)
    cw = fr_words(c)
    us = rand_scalars(2, 8)
    m, k, u_prev = n0, 0, None
    while m >= 2:
        out_l, out_r = np.zeros(8 * n0, dtype=np.uint32), np.zeros(8 * n0, dtype=np.uint32)
        if u_prev is not None:
            s_want = H.key_scalars_fold(s_want, 2 * m, u_prev)
        emu().emu_te_ipa_key_scalars(p32(cw), C.c_size_t(m), p32(s), C.c_size_t(n0), p32(fr_words([u_prev])) if u_prev is not None else None,
                                     C.c_size_t(2 * m if u_prev is not None else 0), p32(out_l), p32(out_r))
        want_l, want_r = H.key_scalars_lr(c, s_want, m)
        assert fr_ints(s) == s_want and fr_ints(out_l) == want_l and fr_ints(out_r) == want_r, m
        u_prev, k, m = us[k], k + 1, m // 2
    emu().emu_te_ipa_key_scalars(None, C.c_size_t(0), p32(s), C.c_size_t(n0), p32(fr_words([u_prev])), C.c_size_t(2), None, None)
    assert fr_ints(s) == H.key_scalars_fold(s_want, 2, u_prev)


# ---- fold table, table fold, out-of-place fold ------------------------------------------------------------------------------------------

def special_key(n_half, u):
    """2 n_half points, multiples of G, with the special entries of the issue in the upper half (where n_half has room for them)"""
    ks = [(i * 0x9e3779b97f4a7c15 + 0xabcdef) ** 3 % E.R for i in range(2 * n_half)]
    key = E.fixed_base(E.GEN).mul_many(ks)
    up = {0: E.T2, 1: E.T4, 2: E.T8, 3: E.add(key[n_half + 3], E.T8) if n_half > 3 else None, 4: E.ZERO}
    for i, p in up.items():
        if i < n_half and p is not None:
            key[n_half + i] = p
    if n_half > 5:
        key[5] = E.neg(E.mul(u, key[n_half + 5]))          # the result is the identity
    if n_half > 6:
        key[6] = E.ZERO
    return key


@pytest.fixture(scope="module")
def table17():
    key = special_key(17, U_SET[-1])
    tbl = np.zeros(H.FOLD_ROWS * 17 * 24, dtype=np.uint32)
    emu().emu_te_ipa_fold_table(p32(resident(key)), C.c_size_t(34), H.FOLD_ROWS, 16, p32(tbl))
    return key, tbl


def test_emu_fold_table_rows(table17):
    key, tbl = table17
    want = H.fold_table(key)
    assert (tbl[:17 * 24] == resident(key)[17 * 24:]).all()                       # row 0 is a copy (the all-zero entry included)
    for b in (1, 2, 3, 100, 252):
        got = [from_resident(tbl[(b * 17 + j) * 24:(b * 17 + j + 1) * 24]) for j in range(17)]
        assert got == want[b], b
    assert want[3][2] == E.IDENT and want[1][4] == E.IDENT                         # 8 T8; the all-zero entry, doubled


@pytest.mark.parametrize("n_half", [1, 15, 16, 17, 128])
def test_emu_fold_from_table_and_ladder(n_half):
    us = U_SET if n_half <= 17 else [U_SET[3], U_SET[-1]]
    tbl = None
    for u in us:
        key = special_key(n_half, u)
        arr = resident(key)
        keep = arr.copy()
        if tbl is None:                                                            # (u only shapes lane 5 of the LOWER half: one table serves every u)
            tbl = np.zeros(H.FOLD_ROWS * n_half * 24, dtype=np.uint32)
            emu().emu_te_ipa_fold_table(p32(arr), C.c_size_t(2 * n_half), H.FOLD_ROWS, 16, p32(tbl))
        want = [E.IDENT if p == E.ZERO else p for p in E.fold(key, u)]
        uw = fr_words([u])
        outs = []
        for t, rows, used_want in ((tbl, H.FOLD_ROWS, 1), (None, 0, 0), (tbl, 8, 1 if u < 64 else 0)):
            out = np.zeros(n_half * 24, dtype=np.uint32)
            used = emu().emu_te_ipa_fold_from(p32(arr), C.c_size_t(n_half), p32(t), rows, p32(uw), 16, p32(out))
            assert used == used_want, (u, rows)
            assert [from_resident(out[24 * i:24 * i + 24]) for i in range(n_half)] == want, (u, rows)
            outs.append(out)
        assert (outs[0] == outs[1]).all() and (outs[1] == outs[2]).all()             # bit for bit
        assert (arr == keep).all()                                                  # src is only read
        if n_half > 5 and u:
            assert want[5] == E.IDENT


def test_emu_subgroup_flags():
    key = E.fixed_base(E.GEN).mul_many(rand_scalars(3, 12))
    key[1] = E.add(key[1], E.T2)
    key[2] = E.T8
    key[3] = E.ZERO
    key[4] = E.IDENT
    key[5] = E.add(key[5], E.T4)
    key[6] = E.T2
    flags = np.full(12, 7, dtype=np.uint32)
    emu().emu_te_ipa_subgroup(p32(resident(key)), C.c_size_t(12), p32(flags))
    want = [1 if E.mul(E.R, p) == E.IDENT else 0 for p in key]
    assert want == [1, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1]
    assert list(flags) == want
    assert not H.in_subgroup(key) and H.in_subgroup(key[7:])


# ---- the built library, no device ------------------------------------------------------------------------------------------------------

def test_library_argument_checks_of_the_new_entry_points():
    from poly_commit_amd import _ffi
    lib = _ffi.load_library()
    INVALID = -1
    null, handle = C.c_void_p(None), C.c_void_p(None)
    buf = np.zeros(64, dtype=np.uint8)
    b_ = buf.ctypes.data_as(C.c_void_p)
    one = C.c_size_t(1)
    assert lib.pc_hip_te_ec_fold_from(null, null, one, b_, C.byref(handle)) == INVALID and handle.value is None
    assert lib.pc_hip_te_srs_precompute_fold(null, null) == INVALID
    rows = C.c_uint(9)
    assert lib.pc_hip_te_srs_fold_table_info(null, C.byref(rows)) == INVALID
    flag = C.c_int(9)
    assert lib.pc_hip_te_srs_in_subgroup(null, null, C.byref(flag)) == INVALID and flag.value == 9
    for curve in (0, 1, -1):
        assert lib.pc_hip_te_fr_powers(null, curve, b_, one, b_) == INVALID
        assert lib.pc_hip_te_ipa_fold_dots(null, curve, b_, b_, one, None, None, b_) == INVALID
        assert lib.pc_hip_te_ipa_key_scalars(null, curve, b_, C.c_size_t(2), b_, C.c_size_t(2), None, C.c_size_t(0), b_, b_) == INVALID
    cb = _ffi.IPA_CHALLENGE_FN(lambda *a: None)
    assert lib.pc_hip_te_ipa_open_rounds(null, null, b_, one, b_, b_, cb, None, C.c_size_t(0), b_, b_, b_, b_, None, None) == INVALID


# ---- the transcript's byte conventions (te_ipa.py and the harness restate them independently) --------------------------------------------

def test_transcript_bytes():
    from poly_commit_amd import te_ipa as D
    ident = np.frombuffer(E.IDENT_BYTES, dtype=np.uint8)
    want = bytes(32) + bytes([1]) + bytes(31)
    assert D.ser_point(ident) == want and H.ser_point(E.IDENT) == want and H.ser_point(E.ZERO) == want
    gx, gy = E.GEN
    want = gx.to_bytes(32, "little") + gy.to_bytes(32, "little")
    assert D.ser_point(E.points_array([E.GEN])[0]) == want and H.ser_point(E.GEN) == want
    assert len(want) == 64 and want[31] < 0x74 and want[63] < 0x74               # canonical residues below q: no flag bits anywhere
    # field elements: canonical little-endian residues in 32 bytes
    assert D.ser_fr(D.fr_from_int(1)) == bytes([1]) + bytes(31) and H.ser_fr(E.R - 1) == (E.R - 1).to_bytes(32, "little")
    assert D.fr_to_int(H.fr_bytes(12345)) == 12345 and H.fr_int(D.fr_from_int(E.R - 2)) == E.R - 2
    # from_random_bytes of the 252-bit field: the top 4 bits of the 32 bytes are cleared, then None at >= r
    for f in (D.from_random_bytes, H.from_random_bytes):
        assert f((E.R - 1).to_bytes(32, "little")) == E.R - 1
        assert f(E.R.to_bytes(32, "little")) is None
        assert f(((1 << 252) - 1).to_bytes(32, "little")) is None
        assert f(((E.R - 1) | (0xf << 252)).to_bytes(32, "little")) == E.R - 1      # only the top 4 bits go
        assert f((5 | (1 << 252)).to_bytes(32, "little")) == 5
        assert f(bytes(32)) == 0
    # the challenge loop retries with the next counter: both restatements agree, and the result is a canonical scalar
    data = b"ed_on_bls12_381 transcript"
    assert D.fr_to_int(D.random_oracle_challenge(data)) == H.challenge(data) < E.R
