"""Case tables and checks of the twisted Edwards probe (tests/hip/probe_field_te.hip, probe_te.hip): shared by
tests/test_te_primitives_cpu.py, which runs them through the host build of the probe, and tests/test_te_primitives_gpu.py, which runs
them on the device and also compares every output word with the host build's.

The references are tests/harness/teref.py (the complete affine law over Python integers) and Python integers; nothing is taken from
the code under test.  The field tables are those of tests/harness/probe.py, loaded the way ref377.probe() loads them: under another
module name, with a private copy of oracle/pyref.py that knows the two fields of ed_on_bls12_381.

Every check takes `probe` (the library under test) and `host` (the host build, the word-for-word twin; the same object in the CPU
suite) and returns its lane count: the tests assert the exact number, so that a table cannot silently shrink.

Conventions of csrc/te.hpp that the expectations restate: the all-zero word pattern is the EMPTY sum (extended words) or the
all-zero base (resident record); as an input it counts as the identity.  empty + empty stays empty, empty + P is P, and a result that
IS the identity is the ordinary value (0, 1): resident words (0, ONE, 0), never all zero."""
import ctypes as C
import functools
import importlib.util
import os
import random

import numpy as np

from harness import teref as E

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FQ, FR = "ed_on_bls12_381_fq", "ed_on_bls12_381_fr"
Q = E.Q
MONT, MONT_INV = E.MONT_Q, pow(E.MONT_Q, -1, E.Q)
FN, XW, AW, XYW = 8, 32, 24, 16
UNSUPPORTED = -1

# probe::TeOp (tests/hip/probe_te_bodies.hpp)
T_MADD, T_ADD, T_DBL, T_TO_AFFINE, T_FROM_AFFINE, T_DERIVE, T_NEG = range(7)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


_probe = None


def probe():
    """tests/harness/probe.py under another module name, its reference a private copy of oracle/pyref.py with the curve's two fields"""
    global _probe
    if _probe is None:
        R = _load("_pyref_ed_on_bls12_381", os.path.join(ROOT, "oracle", "pyref.py"))
        R.FIELDS[FQ] = dict(p=E.Q, limbs64=4)
        R.FIELDS[FR] = dict(p=E.R, limbs64=4)
        _probe = _load("_probe_ed_on_bls12_381", os.path.join(ROOT, "tests", "harness", "probe.py"))
        _probe.R = R
    return _probe


def host_probe():
    return probe().host_probe()


def device_probe():
    return probe().device_probe()


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def twin(name, probe_, host, run):
    """run(library) -> output words; on the device the host build's words must be the same"""
    out = run(probe_)
    if host is not probe_:
        probe().same_words(name, out, run(host))
    return out


# ---- fields ------------------------------------------------------------------------------------------------------------------------

# lanes per group, from the sizes of the operand sets (60 canonical values, 121 lazy ones up to 2p, 120 below 2p, for either field):
# cross products for the binary operations, one lane per member for the unary ones, 1 + 12^4 + 400 tuples for the fused ones
FIELD_LANES = {"products": 60 * 60 + 3 * 60, "fused": 1 + 12 ** 4 + 400, "additive": 2 * 60 * 60 + 2 * 60, "inv": 60}
FIELD_LANES_LAZY = {"lazy_products": 121 * 121 + 121, "lazy_fused": 1 + 12 ** 4 + 400, "lazy_additive": 121 * 121 + 120 + 121 + 60 + 121 + 120 + 121}


def check_field(probe_, host, fname, group):
    return probe().check_field(probe_, host, fname, group)


def lazy_flags(probe_):
    """(LAZY_OK | LAZY_FUSED_OK << 1, LAZY_STORE_OK) per field, as the code under test decides them"""
    return [(probe_.raw("pc_probe_field_lazy_ed_on_bls12_381", C.c_int(w)), probe_.raw("pc_probe_field_lazy_store_ed_on_bls12_381", C.c_int(w)))
            for w in (0, 1)]


# ---- points, representatives, words ------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def point_set():
    """S: multiples of G with two negated ones, the identity, the points of order 2, 4 and 8, a point outside the subgroup, the all-zero entry"""
    G = [E.mul(k, E.GEN) for k in range(1, 6)]
    S = G + [E.neg(G[1]), E.neg(G[3]), E.IDENT, E.T2, E.T4, E.neg(E.T4), E.T8, E.mul(3, E.T8), E.mul(5, E.T8), E.mul(7, E.T8),
             E.add(E.GEN, E.T8), E.ZERO]
    assert len(set(S)) == 17 and all(E.on_curve(p) for p in S[:-1])
    assert {E.mul(2, E.T8), E.mul(6, E.T8)} == {E.T4, E.neg(E.T4)} and E.mul(E.R, S[15]) != E.IDENT
    return tuple(S)


@functools.lru_cache(None)
def lambdas():
    return (1, Q - 1, MONT, (Q - 1) // 2, random.Random(381).randrange(2, Q - 1))


def ext_words(p, lam=1):
    """(lam x, lam y, lam, lam x y) in Montgomery form, 32 words; the all-zero entry is the empty sum"""
    if p == E.ZERO:
        return np.zeros(XW, dtype=np.uint32)
    x, y = p
    return probe().pack([v * MONT % Q for v in (lam * x % Q, lam * y % Q, lam, lam * x % Q * y % Q)], FN).reshape(-1)


@functools.lru_cache(None)
def resident(p):
    """the resident record x | y | 2 d x y of a point (teref.resident_words), all zero for the all-zero entry; read-only, shared"""
    return E.resident_words(p)


def xy_words(p):
    return resident(p)[:XYW]


@functools.lru_cache(None)
def reps():
    """(point, extended words): every real point under every lambda, the point varying fastest, and the empty sum once among them"""
    S = point_set()
    out = [(p, ext_words(p, lam)) for lam in lambdas() for p in S[:-1]]
    out.insert(5, (E.ZERO, ext_words(E.ZERO)))
    assert len(out) == 81
    return tuple(out)


@functools.lru_cache(None)
def esum(p, q):
    """what the additions return: empty + empty is empty, everything else the law's sum (an empty operand counts as the identity)"""
    return E.ZERO if p == E.ZERO and q == E.ZERO else E.add(p, q)


def check_ext(name, row, want):
    """a row of stored extended words stands for `want`: canonical coordinates, Z != 0, T Z = X Y, (X / Z, Y / Z) = want"""
    if want == E.ZERO:
        assert not row.any(), "%s: the empty sum is not all zero: %s" % (name, row)
        return
    raw = probe().unpack(row.reshape(4, FN))
    assert all(v < Q for v in raw), "%s: a coordinate is not below q: %s" % (name, [hex(v) for v in raw])
    X, Y, Z, T = (v * MONT_INV % Q for v in raw)
    assert Z != 0, "%s: Z = 0 on a real point" % name
    assert T * Z % Q == X * Y % Q, "%s: T Z != X Y" % name
    zi = pow(Z, -1, Q)
    got = (X * zi % Q, Y * zi % Q)
    assert got == want, "%s: the stored words are the point %s, want %s" % (name, got, want)


def check_aff(name, row, want):
    """a resident record is exactly x | y | 2 d x y of `want` (all zero for the all-zero entry)"""
    assert np.array_equal(row, resident(want)), "%s: record %s, want %s" % (name, row, resident(want))


# ---- the group law, one primitive per lane -----------------------------------------------------------------------------------------

def run_te(pr, op, Pw, Qw):
    n = len(Pw)
    inp = np.zeros((n, 2 * XW), dtype=np.uint32)
    inp[:, :XW] = Pw
    inp[:, XW:XW + Qw.shape[1]] = Qw
    out = np.zeros((n, XW + AW), dtype=np.uint32)
    pr.call("pc_probe_te", C.c_int(op), C.c_size_t(n), p32(inp), p32(out))
    return out


def _law(probe_, host, name, op, Pw, Qw, wants):
    out = twin("te " + name, probe_, host, lambda pr: run_te(pr, op, Pw, Qw))
    for i, w in enumerate(wants):
        check_ext("te %s lane %d" % (name, i), out[i, :XW], w)
        check_aff("te %s lane %d, to_affine" % (name, i), out[i, XW:], w)
    return len(wants)


def _record(probe_, host, name, op, Qw, wants):
    out = twin("te " + name, probe_, host, lambda pr: run_te(pr, op, np.zeros((len(Qw), XW), dtype=np.uint32), Qw))
    assert not out[:, :XW].any()
    for i, w in enumerate(wants):
        check_aff("te %s lane %d" % (name, i), out[i, XW:], w)
    return len(wants)


def check_madd(probe_, host):
    cases = [(a, b) for a in reps() for b in point_set()]
    return _law(probe_, host, "add_affine", T_MADD, np.array([a[1] for a, _ in cases]), np.array([resident(b) for _, b in cases]),
                [esum(a[0], b) for a, b in cases])


def check_add(probe_, host):
    cases = [(a, b) for a in reps() for b in reps()]
    return _law(probe_, host, "add", T_ADD, np.array([a[1] for a, _ in cases]), np.array([b[1] for _, b in cases]),
                [esum(a[0], b[0]) for a, b in cases])


def check_unary(probe_, host):
    S, rp = point_set(), reps()
    Pw, none = np.array([a[1] for a in rp]), np.zeros((len(rp), 1), dtype=np.uint32)
    n = _law(probe_, host, "dbl", T_DBL, Pw, none, [esum(a[0], a[0]) for a in rp])
    n += _law(probe_, host, "to_affine", T_TO_AFFINE, Pw, none, [a[0] for a in rp])
    Rw = np.array([resident(p) for p in S])
    n += _law(probe_, host, "from_affine", T_FROM_AFFINE, np.zeros((len(S), XW), dtype=np.uint32), Rw, list(S))
    n += _record(probe_, host, "load_xy", T_DERIVE, np.array([xy_words(p) for p in S]), list(S))
    n += _record(probe_, host, "neg_if", T_NEG, Rw, [E.ZERO if p == E.ZERO else E.neg(p) for p in S])
    return n


# ---- chains of mixed additions on one running sum ------------------------------------------------------------------------------------

NEG = 1 << 31
CHAIN_STEPS = 200


def _g(k):
    """the table entry of k G"""
    return k + 5


@functools.lru_cache(None)
def chain_table():
    """entry 0 all zero, 1 the identity, 2..5 = T2, T4, T8, G + T8, entry 5 + k = k G"""
    pts = [E.ZERO, E.IDENT, E.T2, E.T4, E.T8, E.add(E.GEN, E.T8)]
    acc = E.IDENT
    for _ in range(58):
        acc = E.add(acc, E.GEN)
        pts.append(acc)
    assert len(pts) == 64 and pts[_g(3)] == E.mul(3, E.GEN)
    return tuple(pts)


CHAIN_SPECIAL = {
    "only all-zero bases: the sum stays empty": [0, 0 | NEG, 0],
    "an all-zero base on a real sum": [_g(3), 0, 0 | NEG, _g(4)],
    "doubling": [_g(5), _g(5), _g(7)],
    "doubling of a negated digit": [_g(5) | NEG, _g(5) | NEG, _g(9)],
    "P + (-P), then on from the identity": [_g(6), _g(6) | NEG, _g(2), _g(3)],
    "P + (-P): the identity, not empty": [_g(6), _g(6) | NEG],
    "(-P) + P": [_g(6) | NEG, _g(6), _g(2) | NEG],
    "the identity entry alone": [1],
    "low-order entries": [2, 3, 4, 5, 4 | NEG, 3 | NEG, 1, 2, 5 | NEG],
    "T8 eight times: through T4, T2 and the identity": [4] * 8,
    "negated digits": [_g(9) | NEG, _g(4), _g(17) | NEG],
    "doubling deeper in a chain": [_g(1), _g(2), _g(3), _g(6), _g(12), _g(24), _g(48)],            # 1 + 2 = 3: + 3 doubles, + 6 doubles, ...
    "cancelling deeper in a chain": [_g(1), _g(2), _g(3) | NEG, _g(5), _g(5)],
}


def chain_lists():
    """the special lists with three seeded random 200-step lists between them: neighbouring lanes of the one launch take different branches"""
    lists = list(CHAIN_SPECIAL.items())
    for seed in (1, 2, 3):
        rnd = random.Random(seed)
        lists.insert(4 * seed - 2, ("random %d" % seed, [rnd.randrange(64) | (NEG if rnd.random() < 0.5 else 0) for _ in range(CHAIN_STEPS)]))
    return lists


def run_chain(pr, lists, table):
    inp = np.zeros((len(lists), 1 + CHAIN_STEPS), dtype=np.uint32)
    for i, (_, idx) in enumerate(lists):
        inp[i, 0] = len(idx)
        inp[i, 1:1 + len(idx)] = idx
    out = np.zeros((len(lists), 1 + XW + AW), dtype=np.uint32)
    pr.call("pc_probe_te_chain", C.c_size_t(len(lists)), C.c_uint32(CHAIN_STEPS), p32(inp), p32(table), p32(out))
    return out


def check_chain(probe_, host):
    pts = chain_table()
    table = np.array([resident(p) for p in pts]).reshape(-1)
    lists = chain_lists()
    out = twin("te chain (hash of every step's stored words, final sum, its affine form)", probe_, host, lambda pr: run_chain(pr, lists, table))
    for (name, idx), row in zip(lists, out):
        want = E.ZERO
        for e in idx:
            b = pts[e & 63]
            want = esum(want, E.neg(b) if (e & NEG) and b != E.ZERO else b)
        check_ext("te chain '%s'" % name, row[1:1 + XW], want)
        check_aff("te chain '%s', to_affine" % name, row[1 + XW:], want)
    assert [n for (n, idx), row in zip(lists, out) if not row[1:1 + XW].any()] == ["only all-zero bases: the sum stays empty"]
    return len(lists)


# ---- TeBatchAffineBody -------------------------------------------------------------------------------------------------------------------

BATCH_SHAPES = [(1, 1), (1, 16), (15, 16), (16, 16), (17, 16), (33, 16), (40, 7)]
BATCH_VARIANTS = (0, 2, 4)


def batch_cases(n, K, v):
    """n (point, extended words): the real representatives in turn; run t has an empty entry at its start, middle or end, is empty
    throughout, or has none, in that order from variant v on"""
    real = [r for r in reps() if r[0] != E.ZERO]
    out = [real[(7 * v + 3 * j) % len(real)] for j in range(n)]
    empty = (E.ZERO, ext_words(E.ZERO))
    for t in range((n + K - 1) // K):
        s, e = t * K, min(t * K + K, n)
        where = {0: [s], 1: [s + (e - s) // 2], 2: [e - 1], 3: list(range(s, e)), 4: []}[(t + v) % 5]
        for j in where:
            out[j] = empty
    return out


def run_batch(pr, n, K, ext):
    out = np.zeros((n, AW), dtype=np.uint32)
    pr.call("pc_probe_te_batch_affine", C.c_size_t(n), C.c_uint32(K), p32(ext), p32(out))
    return out


def check_batch_affine(probe_, host):
    lanes, kinds = 0, set()
    for n, K in BATCH_SHAPES:
        for v in BATCH_VARIANTS:
            cases = batch_cases(n, K, v)
            ext = np.array([c[1] for c in cases])
            out = twin("te batch_affine n=%d K=%d" % (n, K), probe_, host, lambda pr: run_batch(pr, n, K, ext))
            for j, (p, _) in enumerate(cases):
                check_aff("te batch_affine n=%d K=%d variant %d entry %d" % (n, K, v, j), out[j], E.IDENT if p == E.ZERO else p)
            for t in range((n + K - 1) // K):
                run = [c[0] == E.ZERO for c in cases[t * K:t * K + K]]
                kinds |= {"whole"} if all(run) else {k for k, hit in (("start", run[0]), ("end", run[-1]), ("middle", any(run[1:-1]))) if hit}
            lanes += n
    assert kinds == {"start", "middle", "end", "whole"}
    return lanes


# ---- the fold table and the folds ----------------------------------------------------------------------------------------------------

FOLD_ROWS = 253


@functools.lru_cache(None)
def fold_right():
    """the upper half of the folded key, K of the fold table: 24 entries of S with T8 (T8 -> T4 -> T2 -> identity -> identity) and the
    all-zero record"""
    S = point_set()
    G1, G2, G3, G4, G5, nG2, nG4, I, T2, T4, nT4, T8, T8x3, T8x5, T8x7, GT8, Z = S
    K = (G1, I, I, Z, G2, G3, G4, GT8, T2, G5, T8, T4, nT4, T8x3, T8x5, T8x7, nG2, nG4, Z, I, G1, G2, T8, GT8)
    assert len(K) == 24 and T8 in K and Z in K
    return K


@functools.lru_cache(None)
def fold_table():
    """T[b][j] = 2^b K[j] for b < 253 over Python integers; an all-zero record becomes the identity from the first doubling on"""
    rows = [list(fold_right())]
    for _ in range(FOLD_ROWS - 1):
        rows.append(E._e_affine_batch([E._e_dbl(E._e_from(p)) for p in rows[-1]]))
    j = fold_right().index(E.T8)
    assert [rows[b][j] for b in range(5)][3:] == [E.IDENT, E.IDENT] and rows[2][j] == E.T2 and rows[1][fold_right().index(E.ZERO)] == E.IDENT
    assert rows[252][0] == E.mul(1 << 252, E.GEN)
    return rows


@functools.lru_cache(None)
def fold_table_words():
    return np.array([[resident(p) for p in row] for row in fold_table()], dtype=np.uint32)          # 253 x 24 x 24


def check_row_step(probe_, host):
    """every row of the table from the one below it: ONE TeDblRowBody launch over all (b, j), b < 252, ONE TeBatchAffineBody launch"""
    T, W = fold_table(), fold_table_words()
    half = W.shape[1]
    n = (FOLD_ROWS - 1) * half
    src = np.ascontiguousarray(W[:-1].reshape(n, AW))

    def dbl(pr):
        ext = np.zeros((n, XW), dtype=np.uint32)
        pr.call("pc_probe_te_dbl_row", C.c_size_t(n), p32(src), p32(ext))
        return ext
    ext = twin("te dbl_row", probe_, host, dbl)
    for b in range(FOLD_ROWS - 1):
        for j in range(half):
            check_ext("te dbl_row of T[%d][%d]" % (b, j), ext[b * half + j], E.ZERO if T[b][j] == E.ZERO else T[b + 1][j])
    out = twin("te dbl_row, batch_affine", probe_, host, lambda pr: run_batch(pr, n, 16, ext))
    want = W[1:].reshape(n, AW)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert not len(bad), "row step: T[%d][%d] is %s, want %s" % (bad[0] // half + 1, bad[0] % half, out[bad[0]], want[bad[0]])
    return n


def naf(k):
    """the non-adjacent form of k, least significant digit first"""
    out = []
    while k:
        d = 2 - (k & 3) if k & 1 else 0
        out.append(d)
        k = (k - d) >> 1
    return out


@functools.lru_cache(None)
def fold_scalars():
    r = E.R
    us = (0, 1, 2, 3, 7, r - 1, r - 2, (r - 1) // 2, int("5" * 63, 16), 1 << 251, (1 << 251) + (1 << 250), random.Random(252).randrange(r))
    assert all(0 <= u < r for u in us) and len(set(us)) == 12
    nafs = [naf(u) for u in us]
    assert all(sum(d << i for i, d in enumerate(n)) == u and all(not (a and b) for a, b in zip(n, n[1:])) for n, u in zip(nafs, us))
    assert any(len(n) == FOLD_ROWS for n in nafs), "no u has a digit at position 252, the table's last row"
    assert max(len(n) for n in nafs) <= FOLD_ROWS
    assert any(sum(1 for d in n if d) >= 126 for n in nafs), "no u has 126 non-zero digits"
    return us


def fold_left(u):
    """the lower half for the challenge u: identity or all-zero on the left, the right or both, a doubling (left = u right), a sum that
    is the identity (left = -u right), low-order operands and operands outside the subgroup"""
    S, K = point_set(), fold_right()
    G1, G2, G3, G4, G5, nG2, nG4, I, T2, T4, nT4, T8, T8x3, T8x5, T8x7, GT8, Z = S
    L = [I, G1, I, Z, E.mul(u, K[4]), E.neg(E.mul(u, K[5])), T8, G5, T4, Z, G1, Z, T2, E.mul(u, K[13]), E.neg(E.mul(u, K[14])), GT8, G3, I,
         G1, Z, Z, G4, GT8, T8]
    assert len(L) == len(K)
    return L


def u_words(u):
    return probe().pack([u], 8).reshape(-1)


def check_fold_digits(probe_):
    """TeFoldDigits::from_naf (host code of either build) against the NAF above; a digit at or above `rows` is refused"""
    for u in fold_scalars():
        n = naf(u)
        out = np.zeros(129, dtype=np.uint32)
        assert probe_.raw("pc_probe_te_fold_digits", p32(u_words(u)), C.c_uint32(FOLD_ROWS), p32(out)) == 0, hex(u)
        want = [i | (0x8000 if d < 0 else 0) for i, d in enumerate(n) if d]
        assert out[0] == len(want) and list(out[1:1 + len(want)]) == want, hex(u)
        rows = len(n) - 1          # the top digit has no row
        if rows > 0:
            assert probe_.raw("pc_probe_te_fold_digits", p32(u_words(u)), C.c_uint32(rows), p32(out)) == UNSUPPORTED, (hex(u), rows)
            assert probe_.raw("pc_probe_te_fold_digits", p32(u_words(u)), C.c_uint32(rows + 1), p32(out)) == 0, (hex(u), rows)
    return len(fold_scalars())


def check_folds(probe_, host):
    """ext[i] = L[i] + u Rr[i] by the ladder and from Python's table: both store words of the expected point"""
    K, W = fold_right(), fold_table_words()
    half = len(K)
    tbl = np.ascontiguousarray(W.reshape(-1))
    lanes = 0
    for u in fold_scalars():
        L = fold_left(u)
        want = [E.add(l, E.mul(u, r)) for l, r in zip(L, K)]
        assert want[3] == E.IDENT and (u == 0 or (want[5] == E.IDENT and want[4] == E.mul(2, L[4])))
        key = np.array([resident(p) for p in L + list(K)]).reshape(-1)
        uw = u_words(u)

        def ladder(pr):
            ext = np.zeros((half, XW), dtype=np.uint32)
            pr.call("pc_probe_te_ec_fold", C.c_size_t(half), p32(key), p32(uw), p32(ext))
            return ext

        def tabled(pr):
            ext = np.zeros((half, XW), dtype=np.uint32)
            pr.call("pc_probe_te_table_fold", C.c_size_t(half), p32(key), p32(tbl), C.c_uint32(FOLD_ROWS), C.c_uint32(FOLD_ROWS), p32(uw), p32(ext))
            return ext
        for name, run in (("ec_fold", ladder), ("table_fold", tabled)):
            ext = twin("te %s u=%#x" % (name, u), probe_, host, run)
            for i in range(half):
                check_ext("te %s u=%#x lane %d" % (name, u, i), ext[i], want[i])
            lanes += half
        if len(naf(u)) == FOLD_ROWS:         # a table one row short has no row for the top digit: refused before any launch
            ext = np.zeros((half, XW), dtype=np.uint32)
            assert probe_.raw("pc_probe_te_table_fold", C.c_size_t(half), p32(key), p32(tbl), C.c_uint32(FOLD_ROWS), C.c_uint32(FOLD_ROWS - 1),
                              p32(uw), p32(ext)) == UNSUPPORTED
    return lanes


# ---- subgroup flags, derive and strip ----------------------------------------------------------------------------------------------------

def check_subgroup(probe_, host):
    S = point_set()
    pts = list(S) + [E.add(S[0], E.T2), E.add(S[0], E.T4), E.add(S[1], E.T2), E.add(S[2], E.T4), E.add(S[5], E.T2)]
    want = [1 if p == E.ZERO or E.mul(E.R, p) == E.IDENT else 0 for p in pts]
    assert sum(want) == 9 and len(pts) == 22                # the seven multiples of G, the identity and the all-zero entry
    key = np.array([resident(p) for p in pts]).reshape(-1)

    def run(pr):
        flags = np.zeros((len(pts), 1), dtype=np.uint32)
        pr.call("pc_probe_te_subgroup", C.c_size_t(len(pts)), p32(key), p32(flags))
        return flags
    got = twin("te subgroup flags", probe_, host, run)
    assert [int(f) for f in got[:, 0]] == want, "subgroup flags %s, want %s" % ([int(f) for f in got[:, 0]], want)
    return len(pts)


def check_derive_strip(probe_, host):
    S = point_set()
    xy = np.array([xy_words(p) for p in S])

    def derive(pr):
        out = np.zeros((len(S), AW), dtype=np.uint32)
        pr.call("pc_probe_te_derive", C.c_size_t(len(S)), p32(xy), p32(out))
        return out

    res = twin("te derive", probe_, host, derive)
    for i, p in enumerate(S):
        check_aff("te derive entry %d" % i, res[i], p)

    def strip(pr):
        out = np.zeros((len(S), XYW), dtype=np.uint32)
        pr.call("pc_probe_te_strip", C.c_size_t(len(S)), p32(np.ascontiguousarray(res)), p32(out))
        return out
    back = twin("te strip", probe_, host, strip)
    assert np.array_equal(back, xy), "strip(derive(x | y)) is not x | y"
    return 2 * len(S)
