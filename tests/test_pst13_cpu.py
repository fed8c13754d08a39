"""CPU suite of MarlinPST13: the library's layout helpers against the formula of include/pc_hip.h (a bijection, the tuple order, the
zero-prefix property the design rests on), the limits of the key length, the two restatements of tests/harness/pst13.py -- (A) the
reference's divide_at_point on term dictionaries and (B) the dense fiber definition -- agreeing once constants are set aside, the
reference's identity p(X) - p(z) = sum_i (X_i - z_i) w_i(X) (mod.rs:41), the argument checks of the entry points with no device,
the kernels' bodies stepped on the host (tests/emu/emu_pst13.cpp), and the C++ mirror compiling."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref as R
from harness import pst13 as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = R.FIELDS["bls12_381_fr"]["p"]
SHAPES = [(1, 1), (1, 5), (2, 1), (2, 3), (3, 4), (4, 3), (5, 2), (3, 17), (6, 6)]


def _ffi():
    from poly_commit_amd import _ffi
    _ffi.load_library()
    return _ffi


def rand_terms(n, d, rnd, count=None, p=P):
    """a random term dictionary: `count` distinct monomials of the layout (all of them by default), some coefficients zero"""
    mons = H.monomials(n, d)
    if count is not None:
        mons = rnd.sample(mons, min(count, len(mons)))
    return {e: rnd.randrange(p) for e in mons}


# ---- the layout -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d", SHAPES)
def test_rank_is_the_tuple_order_and_unrank_inverts_it(n, d):
    ffi = _ffi()
    mons = H.monomials(n, d)
    M = len(mons)
    assert ffi.pst13_key_len(n, d) == M == H.key_len(n, d)
    ranks = ffi.pst13_rank(n, d, np.array(mons, dtype=np.uint8))
    assert ranks.tolist() == list(range(M))                        # a bijection onto 0 .. M-1 that equals the tuple order
    assert ranks.tolist() == [H.rank(e, d) for e in mons]         # and the formula of the header
    assert [tuple(r) for r in ffi.pst13_unrank(n, d, np.arange(M, dtype=np.uint32)).tolist()] == mons
    assert [H.unrank(k, n, d) for k in range(M)] == mons
    # the monomials without X_0 .. X_{i-1} are exactly the prefix [0, N(n - i, d)), in the order of the layout (n - i, d)
    for i in range(n + 1):
        zero_prefix = [k for k, e in enumerate(mons) if not any(e[:i])]
        assert zero_prefix == list(range(H.N(n - i, d))), (n, d, i)
        if i < n:
            assert [e[i:] for e in mons[:H.N(n - i, d)]] == H.monomials(n - i, d)
    assert mons[0] == (0,) * n and mons[d] == (0,) * (n - 1) + (d,) and mons[M - 1] == (d,) + (0,) * (n - 1)


def test_key_length_limits():
    ffi = _ffi()
    assert ffi.pst13_key_len(33, 1) == 0 and ffi.pst13_key_len(32, 1) == 33
    assert ffi.pst13_key_len(2, 256) == 0 and ffi.pst13_key_len(2, 255) == 32896
    assert ffi.pst13_key_len(0, 3) == 0 and ffi.pst13_key_len(3, 0) == 0
    assert ffi.pst13_key_len(10, 10) == 184756 and ffi.pst13_key_len(20, 5) == 53130 and ffi.pst13_key_len(8, 16) == 735471
    assert H.N(16, 16) >= 1 << 28 and ffi.pst13_key_len(16, 16) == 0          # M = 601080390
    assert H.N(14, 15) < 1 << 28 and ffi.pst13_key_len(14, 15) == H.N(14, 15)  # 77558760, the largest square-ish shape below the limit
    assert ffi.pst13_key_len(1, (1 << 28) - 2) == (1 << 28) - 1 and ffi.pst13_key_len(1, (1 << 28) - 1) == 0
    # the arithmetic of the issue: pairs the n MSMs of an open cover against n * M
    assert sum(H.N(10 - i, 10) for i in range(10)) == 352715 and 10 * H.N(10, 10) == 1847560
    assert sum(H.N(20 - i, 5) for i in range(20)) == 230229 and 20 * H.N(20, 5) == 1062600


def test_rank_refuses_what_is_outside_the_layout():
    ffi = _ffi()
    with pytest.raises(ffi.PcHipError):
        ffi.pst13_rank(3, 4, np.array([[2, 2, 1]], dtype=np.uint8))         # degree 5
    with pytest.raises(ffi.PcHipError):
        ffi.pst13_unrank(3, 4, np.array([35], dtype=np.uint32))             # M = 35
    with pytest.raises(ffi.PcHipError):
        ffi.pst13_rank(1, 300, np.array([[7]], dtype=np.uint8))             # an exponent is one byte


# ---- (A) == (B) and the reference's identity ------------------------------------------------------------------------------------

def _strip(poly, n):
    return {e: c for e, c in poly.items() if c and any(e)}


@pytest.mark.parametrize("n,d", SHAPES)
def test_term_dictionary_division_equals_the_dense_fibers(n, d):
    rnd = random.Random(0x9513 + 100 * n + d)
    for trial in range(4):
        poly = rand_terms(n, d, rnd, count=None if trial == 0 else rnd.randrange(1, 12))
        if trial == 3:
            poly[next(iter(poly))] = 0                            # a term with coefficient zero
        z = [rnd.randrange(P) for _ in range(n)]
        if trial == 1:
            z[0] = 0
        if trial == 2:
            z = [z[0]] * n
        sparse = H.from_coefficients_vec([(c, e) for e, c in poly.items()], P)
        ws_a = H.divide_at_point(sparse, z, n, P)
        ws_b, value = H.dense_divide(H.to_dense(poly, n, d, P), n, d, z, P)
        assert value == H.evaluate(sparse, z, P)                  # the dense final slot 0 is p(z)
        for i in range(n):
            assert len(ws_b[i]) == H.N(n - i, d)
            wb = {(0,) * i + e: c for e, c in H.from_dense(ws_b[i], n - i, d).items()}
            # the reference drops constants pass by pass: its w_i lacks exactly the part of w_i that comes from them -- the
            # identity below holds for both; term for term they agree wherever the reference kept the dividend's constant out
            assert all(not any(e[:i]) for e in ws_a[i]), "w_i has no variable before X_i"
            at = [rnd.randrange(P) for _ in range(n)]
            assert H.evaluate(wb, at, P) == H.evaluate(ws_a[i], at, P), (n, d, i)
            assert _strip(wb, n) == _strip(ws_a[i], n) and wb.get((0,) * n, 0) == ws_a[i].get((0,) * n, 0)


@pytest.mark.parametrize("n,d", SHAPES)
def test_reference_identity(n, d):
    rnd = random.Random(0x1D + 100 * n + d)
    poly = H.from_coefficients_vec([(c, e) for e, c in rand_terms(n, d, rnd, count=20).items()], P)
    z = [rnd.randrange(P) for _ in range(n)]
    ws, value = H.dense_divide(H.to_dense(poly, n, d, P), n, d, z, P)
    for _ in range(3):
        at = [rnd.randrange(P) for _ in range(n)]
        assert H.check_identity(poly, z, n, at, P)
        rhs = sum((at[i] - z[i]) * H.evaluate(H.from_dense(ws[i], n - i, d), at[i:], P) for i in range(n)) % P
        assert (H.evaluate(poly, at, P) - value) % P == rhs
    assert H.divide_at_point({}, z, n, P) == [{}] * n             # mod.rs:49-51


# ---- the argument checks with no device -------------------------------------------------------------------------------------------

def test_entry_points_check_their_arguments_without_a_device():
    ffi = _ffi()
    lib = ffi.load_library()
    INVALID, TOO_LARGE = -1, -5
    sz = C.c_size_t
    buf = np.zeros(1 << 12, dtype=np.uint8)
    p_ = buf.ctypes.data_as(C.c_void_p)
    szs = (sz * 40)()
    inf = (C.c_int * 40)()
    # a context and a key that are never touched: every check below is made on the arguments alone (the zeroed key belongs to no
    # context, so a call that passes the other checks ends at the key check: PC_ERR_INVALID_ARG as well, still without a device)
    fake = np.zeros(1 << 16, dtype=np.uint8)
    ctx = fake.ctypes.data_as(C.c_void_p)
    fake_key = np.zeros(1 << 12, dtype=np.uint8)
    key = fake_key.ctypes.data_as(C.c_void_p)
    too_large = [(33, 2), (2, 256), (16, 16)]

    def mono(c=ctx, curve=0, n=3, d=4, b=p_, out=p_):
        return lib.pc_hip_pst13_monomial_evals(c, curve, sz(n), sz(d), b, out)
    assert [mono(c=None), mono(b=None), mono(out=None), mono(n=0), mono(d=0), mono(curve=4), mono(curve=-1)] == [INVALID] * 7
    assert [mono(n=n, d=d) for n, d in too_large] == [TOO_LARGE] * 3

    def scatter(c=ctx, curve=0, n=3, d=4, e=p_, co=p_, t=5, out=p_):
        return lib.pc_hip_pst13_scatter(c, curve, sz(n), sz(d), e, co, 0, sz(t), out)
    assert [scatter(c=None), scatter(e=None), scatter(co=None), scatter(out=None), scatter(n=0), scatter(d=0), scatter(curve=9)] == [INVALID] * 7
    assert [scatter(n=n, d=d) for n, d in too_large] == [TOO_LARGE] * 3
    assert scatter(n=1, d=256) == TOO_LARGE and scatter(t=0xFFFFFFFF) == TOO_LARGE

    def divide(c=ctx, curve=0, n=3, d=4, po=p_, z=p_, q=p_, cap=35 + 15 + 5, offs=szs, v=p_):
        return lib.pc_hip_pst13_divide(c, curve, sz(n), sz(d), po, 0, z, q, sz(cap), offs, v)
    assert [divide(c=None), divide(po=None), divide(z=None), divide(q=None), divide(offs=None), divide(v=None)] == [INVALID] * 6
    assert [divide(n=0), divide(d=0), divide(curve=4), divide(cap=35 + 15 + 5 - 1)] == [INVALID] * 4
    assert [divide(n=n, d=d, cap=1 << 40) for n, d in too_large] == [TOO_LARGE] * 3

    def commit(c=ctx, s=key, n=3, d=4, dense=p_, e=None, co=None, t=0, out=p_):
        return lib.pc_hip_pst13_commit(c, s, sz(0), sz(n), sz(d), dense, 0, e, co, 0, sz(t), out, inf)
    assert [commit(c=None), commit(s=None), commit(out=None), commit(n=0), commit(d=0), commit()] == [INVALID] * 6
    assert [commit(e=p_, co=p_, t=3), commit(dense=None, e=None, co=p_, t=3), commit(dense=None, e=p_, co=None, t=3)] == [INVALID] * 3
    assert commit(dense=None, e=p_, co=p_, t=3) == INVALID                            # ends at the key check
    assert [commit(n=n, d=d) for n, d in too_large] == [TOO_LARGE] * 3

    def open_(c=ctx, s=key, n=3, d=4, dense=p_, e=None, co=None, t=0, z=p_, out=p_, v=p_):
        return lib.pc_hip_pst13_open(c, s, sz(0), sz(n), sz(d), dense, 0, e, co, 0, sz(t), z, out, inf, v)
    assert [open_(c=None), open_(s=None), open_(z=None), open_(out=None), open_(v=None), open_(n=0), open_(d=0), open_()] == [INVALID] * 8
    assert [open_(e=p_, co=p_, t=3), open_(dense=None, e=None, co=p_, t=3)] == [INVALID] * 2
    assert [open_(n=n, d=d) for n, d in too_large] == [TOO_LARGE] * 3

    out_key = C.c_void_p(0x1234)

    def trim(c=ctx, s=key, n=3, d=4, sup=2, out=C.byref(out_key)):
        return lib.pc_hip_pst13_trim(c, s, sz(0), sz(n), sz(d), sz(sup), out)
    assert [trim(c=None), trim(s=None), trim(out=None), trim(sup=0), trim(sup=5), trim(n=0), trim()] == [INVALID] * 7
    assert out_key.value is None                                                       # a failed call leaves no key behind
    assert [trim(n=n, d=d) for n, d in too_large] == [TOO_LARGE] * 3
    assert lib.pc_hip_last_pst13_shape(None, None) == INVALID
    assert lib.pc_hip_pst13_rank(sz(3), sz(4), None, sz(1), p_) == INVALID and lib.pc_hip_pst13_unrank(sz(3), sz(4), p_, sz(1), None) == INVALID
    assert lib.pc_hip_pst13_rank(sz(33), sz(4), p_, sz(1), p_) == TOO_LARGE and lib.pc_hip_pst13_unrank(sz(0), sz(4), p_, sz(1), p_) == INVALID


# ---- the kernels' bodies stepped on the host --------------------------------------------------------------------------------------

_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_pst13.so")
        srcs = [os.path.join(HERE, "emu", "emu_pst13.cpp")] + [os.path.join(ROOT, "poly_commit_amd", "csrc", f) for f in ("pst13.hpp", "fp32.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        for f in ("emu_pst13_table_entry", "emu_pst13_unrank", "emu_pst13_rank", "emu_pst13_scatter"):
            getattr(_emu, f).restype = C.c_uint32
        for f in ("emu_pst13_divide", "emu_pst13_monomials", "emu_pst13_rerank"):
            getattr(_emu, f).restype = None
    return _emu


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_binomial_table_and_its_saturation():
    assert all(emu().emu_pst13_table_entry(6, 6, v, r) == H.N(v, r) for v in range(7) for r in range(7))
    assert emu().emu_pst13_table_entry(32, 255, 32, 255) == 0xFFFFFFFF and emu().emu_pst13_table_entry(32, 255, 3, 255) == H.N(3, 255)


@pytest.mark.parametrize("n,d", SHAPES)
def test_unrank_stepped_in_every_sub_layout(n, d):
    """pass i of the division unranks tails in the layout (n - i - 1, d) out of the table of (n, d); trim unranks (n, s) out of it"""
    for nv, budget in sorted({(n - i, d) for i in range(n)} | {(n, s) for s in range(1, d + 1, max(1, d // 3))}):
        mons = H.monomials(nv, budget)
        for k in sorted({0, 1, len(mons) // 2, len(mons) - 1} | set(range(0, len(mons), max(1, len(mons) // 40)))):
            out = np.zeros(max(nv, 1), dtype=np.uint8)
            deg = emu().emu_pst13_unrank(n, d, nv, budget, k, p8(out))
            assert tuple(out[:nv].tolist()) == mons[k] and deg == sum(mons[k]), (n, d, nv, budget, k)
            assert emu().emu_pst13_rank(n, d, nv, budget, p8(out)) == k


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("n,d", [s for s in SHAPES if s[0] >= 2] + [(2, 40)])
def test_division_stepped(curve, n, d):
    fr = R.CURVES[curve]["fr"]
    p = R.FIELDS[fr]["p"]
    rnd = random.Random(0xD1 + 100 * n + d)
    M = H.key_len(n, d)
    for trial in range(2):
        vec = [rnd.randrange(p) for _ in range(M)] if trial == 0 else H.to_dense(rand_terms(n, d, rnd, count=7, p=p), n, d, p)
        z = [rnd.randrange(p) for _ in range(n)]
        if trial == 1:
            z[n - 1] = 0
        want, value = H.dense_divide(vec, n, d, z, p)
        offs = np.cumsum([0] + [len(w) for w in want], dtype=np.uint64)
        quot = np.full((int(offs[-1]) + 1, 4), 0xA5, dtype=np.uint64)
        src = O.fr_mont_array(curve, vec)
        keep = src.copy()
        val = np.zeros(4, dtype=np.uint64)
        emu().emu_pst13_divide(O.CURVES[curve], n, d, p32(src.view(np.uint32)), p32(O.fr_mont_array(curve, z).view(np.uint32)), p32(quot.view(np.uint32)),
                               offs.ctypes.data_as(C.POINTER(C.c_uint64)), p32(val.view(np.uint32)))
        got = O.fr_from_mont_array(curve, quot[:-1])
        assert [got[int(offs[i]):int(offs[i + 1])] for i in range(n)] == want, (n, d)
        assert (quot[-1] == 0xA5).all(), "written past the last quotient"
        assert O.fr_from_mont_array(curve, val.reshape(1, 4)) == [value] and (src == keep).all()


@pytest.mark.parametrize("n,d", SHAPES)
def test_scatter_and_monomials_stepped(n, d):
    curve, p = "bls12_381", P
    rnd = random.Random(0x5CA7 + 100 * n + d)
    M = H.key_len(n, d)
    poly = rand_terms(n, d, rnd, count=min(M, 25))
    poly[next(iter(poly))] = 0
    exps = np.array(list(poly.keys()), dtype=np.uint8).reshape(-1, n)
    co = O.fr_mont_array(curve, list(poly.values()))

    def run(e, c):
        out = np.full((M, 4), 0xA5, dtype=np.uint64)
        flags = emu().emu_pst13_scatter(0, n, d, p8(np.ascontiguousarray(e)), p32(np.ascontiguousarray(c).view(np.uint32)), e.shape[0], p32(out.view(np.uint32)))
        return flags, out
    flags, out = run(exps, co)
    assert flags == 0 and O.fr_from_mont_array(curve, out) == H.to_dense(poly, n, d, p)
    # a repeated tuple is seen with different and with equal coefficients, wherever the two terms are
    for a, b in ((0, exps.shape[0] - 1), (exps.shape[0] // 2, 0)):
        e2, c2 = np.vstack([exps, exps[a:a + 1]]), np.vstack([co, co[b:b + 1]])
        assert run(e2, c2)[0] == 2, "different coefficients"
        c3 = np.vstack([co, co[a:a + 1]])
        assert run(e2, c3)[0] == 2, "equal coefficients"
    over = np.zeros((1, n), dtype=np.uint8)
    over[0, 0] = d + 1
    assert run(np.vstack([exps, over]), np.vstack([co, co[:1]]))[0] == 1
    betas = [rnd.randrange(p) for _ in range(n)]
    pw = O.fr_mont_array(curve, [pow(b, t, p) for b in betas for t in range(d + 1)])
    mono = np.zeros((M, 4), dtype=np.uint64)
    emu().emu_pst13_monomials(0, n, d, p32(pw.view(np.uint32)), p32(mono.view(np.uint32)))
    want = []
    for e in H.monomials(n, d):
        acc = 1
        for b, ej in zip(betas, e):
            acc = acc * pow(b, ej, p) % p
        want.append(acc)
    assert O.fr_from_mont_array(curve, mono) == want


def test_rerank_stepped():
    for n, d, s in ((3, 4, 2), (2, 3, 3), (4, 3, 1), (3, 17, 5)):
        aw = 3
        src = np.arange(H.key_len(n, d) * aw, dtype=np.uint32)
        out = np.zeros(H.key_len(n, s) * aw, dtype=np.uint32)
        emu().emu_pst13_rerank(n, d, s, aw, p32(src), p32(out))
        want = [H.rank(e, d) * aw + w for e in H.monomials(n, s) for w in range(aw)]
        assert out.tolist() == want


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

def test_host_mirror_driver_compiles_and_links():
    """host/marlin_pst13.hpp compiles with -Wall and links against the library; the driver built here is the one the -m gpu test
    runs; without a GPU it refuses cleanly"""
    _ffi()
    libdir = os.path.join(ROOT, "poly_commit_amd")
    exe = os.path.join(HERE, "cpp", "pst13_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no HIP device" in r.stdout
