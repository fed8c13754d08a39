"""CPU-only checks of the twisted Edwards code (csrc/te.hpp: the extended-coordinate law, AccumulateBody / MsmPlan instantiated for
TeOf<ed_on_bls12_381>, the key fold) compiled for the host by tests/emu/emu_te.cpp and stepped lane by lane, against the pure-Python
restatement tests/harness/teref.py.  Every comparison is bit-exact on the affine Montgomery bytes.  The host utilities of the built
library (pc_hip_te_points_sum / pc_hip_te_point_mul), the argument checks and the constants generator need no device either."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from harness import teref as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_te.so")
        srcs = [os.path.join(HERE, "emu", "emu_te.cpp")] + [
            os.path.join(ROOT, "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "ec.hpp", "fp32.hpp", "te.hpp", "te_constants.h", "glv.hpp", "host_tail.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        _emu.emu_te_msm.restype = C.c_int
        _emu.emu_te_accumulate.restype = C.c_uint32
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def xy_words(p):
    return np.frombuffer(E.point_bytes(p), dtype=np.uint32).copy()


def resident(pts):
    return np.concatenate([E.resident_words(p) for p in pts]) if pts else np.zeros(1, dtype=np.uint32)


def from_resident(words):
    """(x, y) of a 24-word resident point, with its third coordinate checked: td = 2 d x y"""
    p = E.point_from_bytes(words[:16].tobytes())
    assert (words == E.resident_words(p)).all(), "the derived coordinate is not 2 d x y"
    return p


def from_extended(words):
    """a 32-word (X, Y, Z, T) bucket -> (x, y), or None for the all-zero (empty) bucket; T Z = X Y is checked"""
    if not words.any():
        return None
    ri = pow(E.MONT_Q, -1, E.Q)
    X, Y, Z, T = (int.from_bytes(words[8 * i:8 * i + 8].tobytes(), "little") for i in range(4))
    assert max(X, Y, Z, T) < E.Q, "a coordinate left [0, q)"
    X, Y, Z, T = (v * ri % E.Q for v in (X, Y, Z, T))
    assert Z != 0 and T * Z % E.Q == X * Y % E.Q
    zi = pow(Z, -1, E.Q)
    return (X * zi % E.Q, Y * zi % E.Q)


@pytest.fixture(scope="module")
def pts():
    return E.fixed_base(E.GEN).mul_many([1, 2, 3, 0x1234567, E.R - 5, 77])


def ecop(op, ext, a, b, aux):
    out = np.zeros(24, dtype=np.uint32)
    emu().emu_te_ecop(op, ext, p32(xy_words(a)), p32(xy_words(b)), p32(xy_words(aux)), p32(out))
    if not out.any():
        return None                       # the empty sum
    return from_resident(out)


def test_te_group_law_all_pairs(pts):
    """Every pair of {subgroup points, a negation, the identity, the points of order 2, 4 and 8, G + T8, the all-zero entry} through the
    mixed and the full addition with Z = 1 and Z != 1, and the doubling: P + P, P + (-P), low-order operands and the identity need no
    special case under the complete law; the all-zero entry counts as the identity (two of them stay the empty sum)."""
    assert all(E.on_curve(p) for p in pts)
    five = pts[:5]
    cand = five + [E.neg(five[2]), E.IDENT, E.T2, E.T4, E.T8, E.add(E.GEN, E.T8), E.ZERO]
    aux = pts[5]
    for ext in (0, 1):
        for a in cand:
            for b in cand:
                if ext and (a == E.ZERO or b == E.ZERO):
                    continue              # (ZERO + X) - X is a real point: covered by a = IDENT
                want = None if (a == E.ZERO and b == E.ZERO) else E.add(a, b)
                assert ecop(0, ext, a, b, aux) == want, (ext, a, b)
                assert ecop(1, ext, a, b, aux) == want, (ext, a, b)
            want = None if a == E.ZERO else E.add(a, a)
            if not (ext and a == E.ZERO):
                assert ecop(2, ext, a, a, aux) == want
        assert ecop(1, 1, five[0], five[1], five[0]) == E.add(five[0], five[1])      # an aux point that collides with the operand


def test_derive_and_strip(pts):
    """x || y -> x || y || 2dxy (the kernel of the upload) and back; the all-zero entry stays all zero"""
    ps = list(pts) + [E.IDENT, E.T2, E.T4, E.T8, E.ZERO]
    xy = np.concatenate([xy_words(p) for p in ps])
    res = np.zeros(24 * len(ps), dtype=np.uint32)
    emu().emu_te_derive(p32(xy), C.c_size_t(len(ps)), p32(res))
    assert (res == resident(ps)).all()
    back = np.zeros_like(xy)
    emu().emu_te_strip(p32(res), C.c_size_t(len(ps)), p32(back))
    assert (back == xy).all()


def test_accumulate_body_on_a_sorted_entry_list(pts):
    """AccumulateBody<TeOf> on a hand-made entry list, chunks of 1 .. 7 entries: an empty bucket (stays all zero), a bucket of all-zero
    bases only (stays all zero too: nothing was added), a bucket that sums to the identity midway (P, -P, then Q: it carries on), a
    bucket that IS the identity at its end, repeated bases (a doubling), low-order bases, and buckets cut by chunk edges.  Per bucket:
    the bucket plus its partials equals the integer-exact sum."""
    P, Qq, S, U = pts[0], pts[1], pts[3], pts[4]
    bases = [P, Qq, S, U, E.ZERO, E.T8, E.add(E.GEN, E.T8), E.T2, E.IDENT, E.T4]
    NEG = 1 << 31
    runs = [
        [0, 1, 2, 3, 0, 1, 2],          # cut by every small chunk length
        [],                             # empty
        [4, 4],                         # only all-zero bases
        [0, 0 | NEG, 1],                # the identity midway
        [2, 2 | NEG],                   # the identity at the end
        [3, 3, 3],                      # doublings
        [5, 6, 7, 8, 9, 5 | NEG, 4],    # low order, the identity and the all-zero entry as bases
        [1 | NEG],
    ]
    entries = np.array([e for r in runs for e in r], dtype=np.uint32)
    offsets = np.cumsum([0] + [len(r) for r in runs]).astype(np.uint32)
    NB = len(runs)
    want = []
    for r in runs:
        acc, real = E.IDENT, False
        for e in r:
            b = bases[e & 0x7fffffff]
            real |= b != E.ZERO
            acc = E.add(acc, E.neg(b) if e & NEG else b)
        want.append(acc if real else None)
    res = resident(bases)
    for T in (1, 2, 3, 5, 7, 64):
        lanes_max = (len(entries) + T - 1) // T
        buckets = np.zeros(NB * 32, dtype=np.uint32)
        pkeys = np.full(2 * lanes_max, 0xffffffff, dtype=np.uint32)
        ppts = np.zeros(2 * lanes_max * 32, dtype=np.uint32)
        lanes = emu().emu_te_accumulate(p32(res), p32(entries), p32(offsets), NB, T, p32(buckets), p32(pkeys), p32(ppts))
        assert lanes == lanes_max
        got = [from_extended(buckets[32 * k:32 * k + 32]) for k in range(NB)]
        cut = set()
        for slot, key in enumerate(pkeys):
            if key == 0xffffffff:
                continue
            part = from_extended(ppts[32 * slot:32 * slot + 32])
            cut.add(int(key))
            if part is not None:
                got[key] = part if got[key] is None else E.add(got[key], part)
        assert got == want, T
        if T == 64:
            assert not cut                     # one chunk: every bucket is complete
        if T == 2:
            assert 0 in cut                    # the first bucket spans four chunks
        assert not buckets[32:64].any() and not buckets[64:96].any()      # the empty ones: all-zero words, not (0, 1, 1, 0)


def run_msm(bases, scalars, n, base_off=0, c=0, T=0, T2=0, K0=0, mont=False):
    b = resident(bases)
    s = E.scalars_array(scalars, mont).view(np.uint32)
    out = np.zeros(16, dtype=np.uint32)
    rc = emu().emu_te_msm(p32(b), C.c_size_t(len(bases)), p32(s), C.c_size_t(n), base_off, c, T, T2, K0, int(mont), p32(out))
    assert rc == 0
    return E.point_from_bytes(out.tobytes())


@pytest.fixture(scope="module")
def key300():
    ks = [(i * 0x9e3779b97f4a7c15 + 12345) ** 3 % E.R for i in range(300)]
    return E.fixed_base(E.GEN).mul_many(ks)


def adversarial_bases(key):
    """the base set of the issue: the identity, an all-zero entry, the points of order 2, 4, 8, P beside -P, a repeated P, and twenty
    points P + T8 outside the prime-order subgroup"""
    b = list(key)
    b[3] = E.IDENT
    b[5] = E.ZERO
    b[7] = E.T2
    b[8] = E.T4
    b[9] = E.T8
    b[11] = E.neg(b[10])
    b[13] = b[12]
    for i in range(20, 40):
        b[i] = E.add(b[i], E.T8)
    return b


def adversarial_scalars(n, seed=3):
    rnd = np.random.RandomState(seed)
    rk = [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]
    return {
        "zeros": [0] * n,
        "ones": [1] * n,
        "r-1": [E.R - 1] * n,
        "same": [rk[0]] * n,
        "two-values": [rk[i % 2] for i in range(n)],
        "carry-chain": [((1 << 252) - 1 - i) % E.R for i in range(n)],
        "sparse": [rk[i] if i % 7 == 0 else 0 for i in range(n)],
    }


SETTINGS = ((0, 0, 0, 0), (6, 4, 4, 2), (9, 7, 5, 4))


@pytest.mark.parametrize("n", [1, 2, 33, 300])
def test_te_msm_stepped(key300, n):
    rnd = np.random.RandomState(n)
    ks = [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]
    want = E.msm(key300[:n], ks)
    for (c, T, T2, K0) in SETTINGS:
        assert run_msm(key300[:n], ks, n, 0, c, T, T2, K0) == want, (c, T, T2, K0)
    assert run_msm(key300[:n], ks, n, 0, 0, 0, 0, 0, mont=True) == want
    if n > 2:      # a base offset, and fewer scalars than bases
        off = 3
        assert run_msm(key300[:n], ks[:n - off], n - off, off, 5, 4, 4, 2) == E.msm(key300[off:n], ks[:n - off])


def test_te_msm_stepped_adversarial(key300):
    """Low-order bases against every scalar set: the digit pipeline is exact integer arithmetic (a use of r P = O would show here)."""
    n = 300
    b = adversarial_bases(key300)
    for name, ks in adversarial_scalars(n).items():
        want = E.msm(b, ks)
        for (c, T, T2, K0) in SETTINGS:
            assert run_msm(b, ks, n, 0, c, T, T2, K0) == want, (name, c, T)
    # the whole sum is the identity: k P + (r - k) P + 8 T8
    ks = [0] * n
    ks[12], ks[13], ks[9] = 12345, E.R - 12345, 8
    assert run_msm(b, ks, n) == E.IDENT == E.msm(b, ks)


@pytest.mark.parametrize("n_half", [1, 2, 17, 65])
def test_te_ec_fold_stepped(key300, n_half):
    """TeEcFoldBody and the batch normalisation: lanes whose left, right or both operands are the identity (or all zero), a doubling,
    a sum that is the identity, low-order operands; u = 0, 1, 2, r - 1 and a random one; the derived coordinate is rebuilt."""
    rnd = np.random.RandomState(n_half)
    us = [0, 1, 2, E.R - 1, int.from_bytes(rnd.bytes(32), "little") % E.R]
    for u in us:
        key = list(key300[:2 * n_half])
        k = key300[100:]
        lanes = {0: (E.IDENT, k[0]), 1: (k[1], E.IDENT), 2: (E.IDENT, E.IDENT), 3: (E.ZERO, E.ZERO), 4: (E.mul(u, k[4]), k[4]),
                 5: (E.neg(E.mul(u, k[5])), k[5]), 6: (E.T8, k[6]), 7: (k[7], E.add(k[8], E.T8)), 8: (E.T4, E.T2), 9: (E.ZERO, k[9])}
        for i, (l, r) in lanes.items():
            if i < n_half:
                key[i], key[n_half + i] = l, r
        want = E.fold(key, u)
        for K in (1, 4, 16):
            arr = resident(key)
            emu().emu_te_fold(p32(arr), C.c_size_t(n_half), p32(E.scalars_array([u], True).view(np.uint32)), K)
            got = [from_resident(arr[24 * i:24 * i + 24]) for i in range(n_half)]
            assert got == want, (u, K)
            assert (arr[24 * n_half:] == resident(key)[24 * n_half:]).all()      # the upper half is left as it was


# ---- the built library, no device ---------------------------------------------------------------------------------------------

def host_points():
    return [E.GEN, E.IDENT, E.T2, E.T4, E.T8, E.add(E.GEN, E.T8)]


def test_library_host_utilities():
    """pc_hip_te_points_sum / pc_hip_te_point_mul against teref: scalars 0, 1, 8, r - 1, r (given as the Montgomery form of r mod r = 0)
    and a 252-bit random one; G, the identity, the points of order 2, 4, 8 and G + T8."""
    from poly_commit_amd import _ffi
    lib = _ffi.load_library()
    pts = host_points()
    out = np.zeros(64, dtype=np.uint8)
    o_ = out.ctypes.data_as(C.c_void_p)
    rnd = np.random.RandomState(252)
    big = (int.from_bytes(rnd.bytes(32), "little") % E.R) | (1 << 251)
    assert big < E.R and big.bit_length() == 252
    for p in pts + [E.ZERO]:
        arr = E.points_array([p])
        for k in (0, 1, 8, E.R - 1, E.R, big):
            ks = E.scalars_array([k % E.R], True)      # the ABI takes one Fr: r itself is the residue 0
            assert lib.pc_hip_te_point_mul(0, arr.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p), o_) == 0
            assert E.point_from_bytes(out.tobytes()) == E.mul(k % E.R, p), (p, k)
    assert E.mul(E.R, E.T8) != E.IDENT      # (the integer r does not annihilate T8; as ONE Fr, which is what this ABI takes, r is the residue 0)
    # sums: every prefix of the list, the list with the all-zero entry and repeats, the empty sum
    seq = pts + [E.ZERO, E.GEN, E.neg(E.GEN), E.T8]
    for cnt in range(len(seq) + 1):
        arr = E.points_array(seq[:cnt]) if cnt else np.zeros((1, 64), dtype=np.uint8)
        assert lib.pc_hip_te_points_sum(0, arr.ctypes.data_as(C.c_void_p), C.c_size_t(cnt), o_) == 0
        want = E.IDENT
        for p in seq[:cnt]:
            want = E.add(want, p)
        assert E.point_from_bytes(out.tobytes()) == want, cnt
        if want == E.IDENT:
            assert out.tobytes() == E.IDENT_BYTES
    # the convenience wrappers
    assert E.point_from_bytes(_ffi.te_points_sum("ed_on_bls12_381", E.points_array(pts)).tobytes()) == E.msm(pts, [1] * len(pts))
    assert E.point_from_bytes(_ffi.te_point_mul("ed_on_bls12_381", E.points_array([E.T8])[0], E.scalars_array([5], True)[0]).tobytes()) == E.mul(5, E.T8)


def test_library_argument_checks():
    """Every argument check of the pc_hip_te_* entry points, an unknown pc_te_curve included, with no device."""
    from poly_commit_amd import _ffi
    lib = _ffi.load_library()
    assert _ffi.TE_CURVES == {"ed_on_bls12_381": 0}
    arr = E.points_array(host_points())
    ks = E.scalars_array([5], True)
    out = np.zeros(64, dtype=np.uint8)
    p_, k_, o_ = arr.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    INVALID = -1
    assert lib.pc_hip_te_points_sum(0, None, C.c_size_t(2), o_) == INVALID
    assert lib.pc_hip_te_points_sum(0, p_, C.c_size_t(2), None) == INVALID
    assert lib.pc_hip_te_points_sum(0, None, C.c_size_t(0), o_) == 0 and out.tobytes() == E.IDENT_BYTES      # the empty sum needs no points
    assert lib.pc_hip_te_point_mul(0, None, k_, o_) == INVALID
    assert lib.pc_hip_te_point_mul(0, p_, None, o_) == INVALID
    assert lib.pc_hip_te_point_mul(0, p_, k_, None) == INVALID
    for curve in (1, 3, 4, -1):           # no other twisted Edwards curve; the ids of pc_curve mean nothing here
        assert lib.pc_hip_te_points_sum(curve, p_, C.c_size_t(2), o_) == INVALID
        assert lib.pc_hip_te_point_mul(curve, p_, k_, o_) == INVALID
    # entry points that take a context or a key refuse NULL before the device is touched
    null = C.c_void_p(None)
    handle = C.c_void_p(None)
    assert lib.pc_hip_te_srs_upload(null, 0, p_, C.c_size_t(1), C.c_size_t(0), 0, C.byref(handle)) == INVALID
    assert lib.pc_hip_te_srs_upload(null, 1, p_, C.c_size_t(1), C.c_size_t(0), 0, C.byref(handle)) == INVALID
    assert lib.pc_hip_te_srs_upload(null, 0, p_, C.c_size_t(1), C.c_size_t(0), 0, None) == INVALID
    assert handle.value is None
    assert lib.pc_hip_te_msm(null, null, C.c_size_t(0), k_, 1, 0, C.c_size_t(1), o_, None) == INVALID
    assert lib.pc_hip_te_ec_fold(null, null, C.c_size_t(1), k_) == INVALID
    assert lib.pc_hip_te_srs_read(null, null, C.c_size_t(0), C.c_size_t(0), o_) == INVALID
    four = (C.c_size_t * 4)()
    assert lib.pc_hip_te_srs_bytes_resident(null, four) == INVALID
    assert lib.pc_hip_te_srs_len(null) == 0
    lib.pc_hip_te_srs_free(null)


def test_constants_generator_reproduces_the_header():
    """tools/gen_te_constants.py (which asserts the curve facts before it writes anything) prints the committed csrc/te_constants.h"""
    got = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_te_constants.py"), "--stdout"])
    with open(os.path.join(ROOT, "poly_commit_amd", "csrc", "te_constants.h"), "rb") as fh:
        assert got == fh.read()
