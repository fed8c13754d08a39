"""The contract of the MSM's bucket reduction in Python integers over logarithms, for tests/test_msm_reduce_gpu.py and
tests/test_msm_reduce_cpu.py (the probe unit tests/hip/probe_reduce.hip).

Every input point is e G for a known e: a member of the signedkey pool (8 seeded logarithms, both signs) or the infinity (e = 0), in
XYZZ words, as (x, y, 1, 1) or as a random representative (x lam^2, y lam^3, lam^2, lam^3).  What a level or a whole reduction must
put out is then a sum of logarithms, and the point it stands for is (that sum mod r) G: integers and ONE multiplication of the
generator per output point (by a fixed-base table of the Python reference's own group law).  No bucket method has a part in it.

The level contract (comments of BucketLevelBody / BucketLevelBitsBody, csrc/msm.hpp), arrays of cnt points each, group g of K inputs:
  array 0                S_g = sum_l X[g][l]
  mode 0:  array 1       sum_l (l + weight_off) X[g][l];   arrays 2 ..       the plain sums of the older arrays
  modes 1, 2: array 1+b  A_b = sum over the l with bit b set of X[g][l];   array 1 + lgK: a copy of S when weight_off;
           arrays nw + 1 .. (nw = lgK + weight_off): the plain sums of the older arrays
The plan (`plan`): msm_make_geom and msm_plan_levels restated.  The whole reduction: for every bucket set w,
sum_a 2^arr_exp[a] out_a[w] = sum_j (j + 1) B[w][j].
"""
import ctypes as C
import random

import numpy as np

import oracle_lib as O
from harness import g2ref as G2
from harness import signedkey as SK
from harness import sortref as S
from harness.probe import p32

GROUPS = ["bls12_381", "bn254", "pallas", "bls12_377", "bls12_381_g2"]      # the probe's group ids
BAD_OP = -2
PLAN_WORDS = 200
MAX_POINTS = 1 << 21
ZERO_KNOB = (1 << 64) - 1              # a knob of 0 keeps the default; this one sets the field to 0
KNOBS = ("K0", "tbl_K0", "K1", "coop_max_points", "coop2_max_points", "coop2_max_entries")
NREP = 5                               # representatives per pool point: (x, y, 1, 1) and four random ones


# ---- groups ------------------------------------------------------------------------------------------------------------------------

class FixedG1:
    """t G for many t: 32 windows of 8 bits, table[w][d - 1] = d 2^(8 w) G, by the reference's affine addition"""

    def __init__(self, ref, curve):
        self.ref, self.curve, self.tbl = ref, curve, []
        cur = ref.generator(curve)
        for _ in range(32):
            row, acc = [], None
            for _d in range(255):
                acc = ref.ec_add(curve, acc, cur)
                row.append(acc)
            self.tbl.append(row)
            cur = ref.ec_add(curve, acc, cur)

    def mul(self, t):
        acc = None
        for w in range(32):
            d = (t >> (8 * w)) & 0xff
            if d:
                acc = self.ref.ec_add(self.curve, acc, self.tbl[w][d - 1])
        return acc


class Group:
    _made = {}

    def __new__(cls, name):
        if name not in cls._made:
            cls._made[name] = super().__new__(cls)
            cls._made[name]._init(name)
        return cls._made[name]

    def _init(self, name):
        self.name, self.id, self.g2 = name, GROUPS.index(name), name.endswith("_g2")
        self.curve = name[:-3] if self.g2 else name
        ref = self.ref = O.ref(self.curve)
        fq = ref.FIELDS[ref.CURVES[self.curve]["fq"]]
        self.p, self.N = fq["p"], 2 * fq["limbs64"]
        self.R = 1 << (32 * self.N)
        self.Ri = pow(self.R, -1, self.p)
        self.r = ref.FIELDS[ref.CURVES[self.curve]["fr"]]["p"]
        self.bits = S.FR_BITS[self.curve]
        self.FN = self.N * (2 if self.g2 else 1)
        self.PW = 4 * self.FN
        self.ks = SK.pool(self.curve)[0]
        # fp32.hpp LAZY_STORE_OK: a stored coordinate may lie anywhere below 2p where R >= 9p (the 12-limb G1 curves); elsewhere, and
        # over Fq2, the stored form is canonical
        self.lazy_store = (not self.g2) and self.N > 8 and ((self.p >> (32 * (self.N - 1))) + 1) * 9 <= 1 << 32
        self.glv = not self.g2
        self._fixed, self._mul, self._reps = None, {0: None}, None

    # logarithm -> point
    def mul_g(self, t):
        t %= self.r
        if t not in self._mul:
            if self._fixed is None:
                self._fixed = G2.fixed_base(G2.generator()) if self.g2 else FixedG1(self.ref, self.curve)
            self._mul[t] = self._fixed.mul_many([t])[0] if self.g2 else self._fixed.mul(t)
        return self._mul[t]

    def mul_g_slow(self, t):
        """the same by the reference's own scalar multiplication (the fixed-base table is held against it)"""
        t %= self.r
        if not t:
            return None
        return G2.mul(t, G2.generator()) if self.g2 else self.ref.ec_mul(self.curve, t, self.ref.generator(self.curve))

    # coordinates <-> words
    def cmul(self, a, b):
        return G2.f2_mul(a, b) if self.g2 else a * b % self.p

    def cinv(self, a):
        return G2.f2_inv(a) if self.g2 else pow(a, -1, self.p)

    def enc(self, c):
        vals = [x * self.R % self.p for x in (c if self.g2 else (c,))]
        return np.frombuffer(b"".join(v.to_bytes(4 * self.N, "little") for v in vals), dtype=np.uint32)

    def dec(self, w):
        raw = np.ascontiguousarray(w).tobytes()
        v = [int.from_bytes(raw[4 * self.N * i:4 * self.N * (i + 1)], "little") * self.Ri % self.p for i in range(len(w) // self.N)]
        return tuple(v) if self.g2 else v[0]

    def words(self, A, lam=None):
        """X | Y | ZZ | ZZZ; lam: the representative (x lam^2, y lam^3, lam^2, lam^3)"""
        if A is None:
            return np.zeros(self.PW, dtype=np.uint32)
        one = (1, 0) if self.g2 else 1
        l1 = one if lam is None else lam
        l2 = self.cmul(l1, l1)
        l3 = self.cmul(l2, l1)
        return np.concatenate([self.enc(self.cmul(A[0], l2)), self.enc(self.cmul(A[1], l3)), self.enc(l2), self.enc(l3)])

    def affine_of(self, w):
        """the point a row of XYZZ words stands for (lazily reduced coordinates included); ZZ = 0 is the infinity; checks ZZ^3 = ZZZ^2"""
        FN = self.FN
        if not w[2 * FN:3 * FN].any():
            return None
        X, Y, ZZ, ZZZ = (self.dec(w[k * FN:(k + 1) * FN]) for k in range(4))
        assert ZZ != ((0, 0) if self.g2 else 0), "ZZ is a non-zero multiple of p"
        assert self.cmul(self.cmul(ZZ, ZZ), ZZ) == self.cmul(ZZZ, ZZZ), "ZZ^3 != ZZZ^2"
        return (self.cmul(X, self.cinv(ZZ)), self.cmul(Y, self.cinv(ZZZ)))

    def lam(self, rnd):
        return (rnd.randrange(1, self.p), rnd.randrange(self.p)) if self.g2 else rnd.randrange(1, self.p)

    def reps(self):
        """(17, NREP, PW) words: rows +Q_0 .. +Q_7, -Q_0 .. -Q_7, infinity (signedkey's order); column 0 has ZZ = ZZZ = 1"""
        if self._reps is None:
            rnd = random.Random(0xBEEF + self.id)
            t = np.zeros((2 * SK.POOL + 1, NREP, self.PW), dtype=np.uint32)
            for i, e in enumerate(self.pool_logs()[:-1]):
                A = self.mul_g(e)
                for k in range(NREP):
                    t[i, k] = self.words(A, self.lam(rnd) if k else None)
            self._reps = t
        return self._reps

    def pool_logs(self):
        return list(self.ks) + [self.r - k for k in self.ks] + [0]

    def plus_p(self, w):
        """the same points with p added to every coordinate of every finite one: below 2p, the most the stored form allows"""
        assert self.lazy_store
        rows = w.reshape(-1, self.PW)
        out = rows.copy()
        N = self.N
        for i, row in enumerate(rows):
            if not row[2 * self.FN:3 * self.FN].any():
                continue
            raw = row.tobytes()
            vals = [int.from_bytes(raw[4 * N * k:4 * N * (k + 1)], "little") for k in range(4)]
            assert all(v < self.p for v in vals)
            out[i] = np.frombuffer(b"".join((v + self.p).to_bytes(4 * N, "little") for v in vals), dtype=np.uint32)
        return out.reshape(w.shape)


# ---- bucket contents ---------------------------------------------------------------------------------------------------------------
# a content is (idx, rep): two integer arrays of one shape; idx the row of the pool table, rep the representative

INF = 2 * SK.POOL


def gather(g, idx, rep):
    return np.ascontiguousarray(g.reps()[idx, rep])


def logs_of(g, idx):
    table = np.array(g.pool_logs(), dtype=object)
    return table[idx]


CONTENTS = ("random", "equal_same_words", "equal_other_words", "alternating", "alternating_pairs", "all_infinite", "single_last", "lazy")


def content(name, shape, seed):
    """-> (idx, rep) of `shape` (.., K): the last axis runs along a group"""
    rnd = np.random.RandomState(seed)
    K = shape[-1]
    l = np.broadcast_to(np.arange(K), shape)
    if name in ("random", "lazy"):
        idx = rnd.randint(0, 2 * SK.POOL, size=shape)
        idx[rnd.randint(0, 9, size=shape) == 0] = INF           # about one place in nine at infinity
        return idx, rnd.randint(0, NREP, size=shape)
    q = int(rnd.randint(0, SK.POOL))
    if name == "equal_same_words":
        return np.full(shape, q), np.full(shape, 1 + seed % (NREP - 1))
    if name == "equal_other_words":
        return np.full(shape, q), np.array(l % NREP)
    if name == "alternating":                                    # Q, -Q, Q, -Q: the first tree step cancels everywhere
        return q + SK.POOL * (l & 1), rnd.randint(0, NREP, size=shape)
    if name == "alternating_pairs":                              # Q, Q, -Q, -Q: the first step doubles, the second cancels
        return q + SK.POOL * ((l >> 1) & 1), rnd.randint(0, NREP, size=shape)
    if name == "all_infinite":
        return np.full(shape, INF), np.zeros(shape, dtype=np.int64)
    if name == "single_last":
        idx = np.full(shape, INF)
        idx[..., K - 1] = q
        return idx, np.full(shape, 2)
    raise KeyError(name)


# ---- one level ---------------------------------------------------------------------------------------------------------------------

def lg(K):
    assert K >= 1 and K & (K - 1) == 0
    return K.bit_length() - 1


def level_arrays(K, woff, n_old, mode):
    """arrays of the level, S included"""
    return 1 + (lg(K) + woff if mode else 1) + n_old


def expected_level(r, K, woff, n_old, mode, xlogs, oldlogs):
    """xlogs: (cnt, K) logarithms; oldlogs: (n_old, cnt, K) -> list of arrays, each a list of cnt logarithms mod r"""
    cnt = len(xlogs)
    S_ = [sum(row) % r for row in xlogs]
    out = [S_]
    if mode == 0:
        out.append([sum((l + woff) * int(e) for l, e in enumerate(row)) % r for row in xlogs])
    else:
        for b in range(lg(K)):
            out.append([sum(int(e) for l, e in enumerate(row) if (l >> b) & 1) % r for row in xlogs])
        if woff:
            out.append(list(S_))
    for a in range(n_old):
        out.append([sum(oldlogs[a][g]) % r for g in range(cnt)])
    assert len(out) == level_arrays(K, woff, n_old, mode)
    return out


def run_level(probe, g, K, woff, cnt, n_old, mode, xw, oldw):
    """-> (arrays + 1, cnt, PW) words: the level's arrays and the cnt points behind them"""
    na = level_arrays(K, woff, n_old, mode)
    out = np.zeros(((na + 1) * cnt, g.PW), dtype=np.uint32)
    oldw = oldw if n_old else np.zeros((1, g.PW), dtype=np.uint32)
    probe.call("pc_probe_reduce_level", g.id, C.c_uint32(K), C.c_uint32(woff), C.c_uint32(cnt), C.c_uint32(n_old), C.c_int(mode),
               p32(np.ascontiguousarray(xw)), p32(np.ascontiguousarray(oldw)), p32(out), C.c_size_t(len(out)))
    return out.reshape(na + 1, cnt, g.PW)


def check_points(g, got, want_logs, what):
    """got: (n, PW) words; want_logs: n logarithms.  The infinity is ZZ = 0; a finite point is compared as a point"""
    assert len(got) == len(want_logs), what
    for i, (w, t) in enumerate(zip(got, want_logs)):
        want = g.mul_g(int(t))
        have = g.affine_of(w)
        if want is None:
            assert have is None and not w.any(), "%s: point %d should be the infinity, all-zero words" % (what, i)
        else:
            assert have == want, "%s: point %d is %s" % (what, i, "the infinity" if have is None else "another point")


def check_level(g, out, want, what):
    """out: run_level's words; want: expected_level's logarithms.  Every array, and the preset behind the last one"""
    na, cnt = len(want), out.shape[1]
    assert out.shape[0] == na + 1
    for a in range(na):
        check_points(g, out[a], want[a], "%s, array %d" % (what, a))
    assert (out[na] == 0xffffffff).all(), "%s: a write behind the level's arrays" % what
    return na * cnt


def level_case(g, name, K, cnt, n_old, seed):
    """-> (x words (cnt K, PW), old words (n_old cnt K, PW), x logs (cnt, K), old logs (n_old, cnt, K))"""
    xi, xr = content(name, (cnt, K), seed)
    oi, orp = content(name, (n_old, cnt, K), seed + 1)
    xw, ow = gather(g, xi, xr).reshape(-1, g.PW), gather(g, oi, orp).reshape(-1, g.PW)
    if name == "lazy":
        xw, ow = g.plus_p(xw), g.plus_p(ow)
    return xw, ow, logs_of(g, xi), logs_of(g, oi)


def one_hot_case(g, K, n_old, seed):
    """cnt = K groups, group j holds one pool point at l = j and the infinity elsewhere; the same in ONE older array (the last)"""
    rnd = np.random.RandomState(seed)
    j = np.arange(K)

    def hot():
        idx = np.full((K, K), INF)
        idx[j, j] = rnd.randint(0, 2 * SK.POOL, size=K)
        return idx, rnd.randint(0, NREP, size=(K, K))
    xi, xr = hot()
    oi, orp = np.full((n_old, K, K), INF), np.zeros((n_old, K, K), dtype=np.int64)
    if n_old:
        oi[n_old - 1], orp[n_old - 1] = hot()
    return gather(g, xi, xr).reshape(-1, g.PW), gather(g, oi, orp).reshape(-1, g.PW), xi, oi


def check_one_hot(g, out, K, woff, n_old, mode, xw, ow, what):
    """every output is one input's words, a multiple the serial weights ask for, or all-zero words: word for word where no
    arithmetic is involved (weight 0 or 1), as a point where mode 0 multiplies (l + weight_off) X"""
    na = level_arrays(K, woff, n_old, mode)
    xw, zero = xw.reshape(K, K, g.PW), np.zeros(g.PW, dtype=np.uint32)
    hot = [xw[j, j] for j in range(K)]
    want = [hot]
    if mode == 0:
        want.append(None)
    else:
        for b in range(lg(K)):
            want.append([hot[j] if (j >> b) & 1 else zero for j in range(K)])
        if woff:
            want.append(hot)
    for a in range(n_old):
        o = ow.reshape(n_old, K, K, g.PW)[a]
        want.append([o[j, j] for j in range(K)])
    assert len(want) == na
    for a in range(na):
        if want[a] is None:
            for j in range(K):
                wt = j + woff
                base = g.affine_of(hot[j])
                pt = None
                for _ in range(wt):
                    pt = G2.add(pt, base) if g.g2 else g.ref.ec_add(g.curve, pt, base)
                assert g.affine_of(out[a, j]) == pt, "%s: one-hot, weighted array, group %d" % (what, j)
                if wt == 0:
                    assert not out[a, j].any()
                if wt == 1:
                    assert (out[a, j] == hot[j]).all()
        else:
            assert (out[a] == np.array(want[a])).all(), "%s: one-hot, array %d" % (what, a)
    assert (out[na] == 0xffffffff).all(), "%s: a write behind the level's arrays" % what
    return na * K


# ---- the plan ----------------------------------------------------------------------------------------------------------------------

DEFAULTS = {"K0": 8, "tbl_K0": 8, "K1": 256, "coop_max_points": 1 << 17, "coop2_max_points": 1 << 15, "coop2_max_entries": 1 << 22}


def _pow2_floor(v, lo, hi):
    p = lo
    while p * 2 <= v and p * 2 <= hi:
        p *= 2
    return p


class Plan:
    def __init__(self, W, Wd, nb_win, levels, arr_exp):
        self.W, self.Wd, self.nb_win, self.levels, self.arr_exp = W, Wd, nb_win, levels, arr_exp      # levels: (K, mode, m, narr)

    def key(self):
        return (self.W, self.Wd, self.nb_win, tuple(self.levels), tuple(self.arr_exp))

    def tuples(self):
        """(K, mode, weight_off, n_old) of every level"""
        return [(K, mode, 1 if l == 0 else 0, self.levels[l - 1][3] if l else 0) for l, (K, mode, _, _) in enumerate(self.levels)]


def plan(g, n, c, tbl=0, glv=0, subs=0, **knobs):
    """msm_make_geom and msm_plan_levels (csrc/msm.hpp) under the group's default MsmConfig, restated"""
    cfg = dict(DEFAULTS)
    if g.g2:
        cfg["K1"], cfg["coop2_max_points"] = 128, 0
    cfg.update(knobs)
    cfg["K0"], cfg["tbl_K0"], cfg["K1"] = _pow2_floor(cfg["K0"], 2, 1 << 12), _pow2_floor(cfg["tbl_K0"], 2, 1 << 12), _pow2_floor(cfg["K1"], 2, 256)
    windows = (S.HALF_BITS if glv else g.bits) // c + 1
    Wd = 2 * windows if glv else windows
    W = subs * (2 if glv else 1) if subs else (2 if glv else 1) if tbl else Wd
    nb_win = 1 << (c - 1)
    m, kbits, levels, arr_exp = nb_win, 0, [], []
    while m > 1:
        prev = levels[-1][3] if levels else 0
        level_pts = W * m * (1 + prev) if n * Wd <= cfg["coop2_max_entries"] else None
        two = level_pts is not None and level_pts <= cfg["coop2_max_points"]
        if W * m > cfg["coop_max_points"]:
            K = cfg["tbl_K0"] if tbl else cfg["K0"]
        else:
            rem = (m - 1).bit_length()
            lg1 = (cfg["K1"] - 1).bit_length()
            if two and lg1 > 7:
                lg1 = 7
            nl = (rem + lg1 - 1) // lg1
            K = 1 << ((rem + nl - 1) // nl)
        K = min(K, m)
        lgK = lg(K)
        bits = K >= 16
        woff = 0 if levels else 1
        nw = lgK + woff if bits else 1
        m //= K
        mode = 0 if not bits else 2 if (K <= 128 and two) else 1
        levels.append((K, mode, m, nw + prev))
        new = [kbits + b for b in range(lgK)] + ([kbits] if woff else []) if bits else [kbits]
        arr_exp = new + arr_exp
        kbits += lgK
    return Plan(W, Wd, nb_win, levels, arr_exp)


def knob_array(knobs):
    a = np.zeros(6, dtype=np.uint64)
    for k, v in knobs.items():
        a[KNOBS.index(k)] = ZERO_KNOB if v == 0 else v
    return a


def probe_plan(probe, g, n, c, tbl=0, glv=0, subs=0, **knobs):
    """the plan pc_probe_reduce_plan reports, or BAD_OP"""
    out, kn = np.zeros(PLAN_WORDS, dtype=np.uint32), knob_array(knobs)
    st = probe.raw("pc_probe_reduce_plan", g.id, C.c_size_t(n), C.c_uint32(c), C.c_uint32(tbl), C.c_uint32(glv), C.c_uint32(subs),
                   kn.ctypes.data_as(C.POINTER(C.c_uint64)), p32(out))
    if st != 0:
        assert st == BAD_OP, st
        return BAD_OP
    L = int(out[3])
    levels = [tuple(int(v) for v in out[4 + 4 * l:8 + 4 * l]) for l in range(L)]
    return Plan(int(out[0]), int(out[1]), int(out[2]), levels, [int(v) for v in out[133:133 + int(out[132])]])


# ---- the whole reduction -----------------------------------------------------------------------------------------------------------

def run_all(probe, g, pl, n, c, tbl, glv, subs, buckets, **knobs):
    """-> (arrays (narr, W, PW), fold (W, PW) or None)"""
    narr = pl.levels[-1][3]
    arrays = np.zeros((narr * pl.W, g.PW), dtype=np.uint32)
    fold = np.full((pl.W, g.PW), 0xffffffff, dtype=np.uint32)
    kn = knob_array(knobs)
    probe.call("pc_probe_reduce_all", g.id, C.c_size_t(n), C.c_uint32(c), C.c_uint32(tbl), C.c_uint32(glv), C.c_uint32(subs),
               kn.ctypes.data_as(C.POINTER(C.c_uint64)), p32(np.ascontiguousarray(buckets)), p32(arrays), p32(fold))
    return arrays.reshape(narr, pl.W, g.PW), (fold if subs else None)


def expected_all(g, pl, blogs):
    """blogs: (W, nb_win) logarithms of the buckets -> per bucket set sum_j (j + 1) B[w][j] mod r"""
    return [sum((j + 1) * int(e) for j, e in enumerate(row)) % g.r for row in blogs]


def combine(g, pl, arrays, exps=None):
    """sum_a 2^exp[a] out_a[w] per bucket set, by the reference's own group law (doublings and additions; G2 in the reference's
    Jacobian form with one normalisation at the end)"""
    exps = pl.arr_exp if exps is None else exps
    assert len(exps) == arrays.shape[0]
    if g.g2:
        lift, add, dbl = (lambda A: G2._j_from(A)), G2._j_add, G2._j_dbl
        zero, done = G2._J_INF, G2._j_affine_batch
    else:
        lift, add, dbl = (lambda A: A), (lambda A, B: g.ref.ec_add(g.curve, A, B)), (lambda A: g.ref.ec_add(g.curve, A, A))
        zero, done = None, list
    order = sorted(range(len(exps)), key=lambda a: -exps[a])
    out = []
    for w in range(arrays.shape[1]):
        acc, cur = zero, exps[order[0]]
        for a in order:
            while cur > exps[a]:
                acc, cur = dbl(acc), cur - 1
            acc = add(acc, lift(g.affine_of(arrays[a, w])))
        while cur > 0:
            acc, cur = dbl(acc), cur - 1
        out.append(acc)
    return done(out)


def check_all(g, pl, arrays, fold, blogs, what, exps=None):
    """every bucket set's weighted sum of the output arrays is (sum_j (j + 1) log B[w][j]) G; the device's own fold (many-MSM mode) too"""
    want = [g.mul_g(t) for t in expected_all(g, pl, blogs)]
    got = combine(g, pl, arrays, exps)
    for w, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s: bucket set %d" % (what, w)
    if fold is not None:
        for w, b in enumerate(want):
            assert g.affine_of(fold[w]) == b, "%s: SubFoldBody, bucket set %d" % (what, w)
            if b is None:
                assert not fold[w][2 * g.FN:3 * g.FN].any()
    return len(want)


def run_whole(probe, g, call, name, seed, what=None):
    """one whole reduction over buckets of content `name`; call = (n, c, tbl, glv, subs, knobs) -> points checked"""
    n, c, tbl, glv, subs, knobs = call
    pl = probe_plan(probe, g, n, c, tbl, glv, subs, **knobs)
    assert pl != BAD_OP and pl.key() == plan(g, n, c, tbl, glv, subs, **knobs).key(), (g.name, call)
    idx, rep = content(name, (pl.W, pl.nb_win), seed)
    arrays, fold = run_all(probe, g, pl, n, c, tbl, glv, subs, gather(g, idx, rep).reshape(-1, g.PW), **knobs)
    return check_all(g, pl, arrays, fold, logs_of(g, idx), what or "%s %r %s" % (g.name, call, name))


def run_whole_one_hot(probe, g, call, seed):
    """bucket set w holds ONE finite bucket, j = w + k W in run k: every bucket of a set is the lone one once"""
    n, c, tbl, glv, subs, knobs = call
    pl = plan(g, n, c, tbl, glv, subs, **knobs)
    rnd = np.random.RandomState(seed)
    done = 0
    for k in range((pl.nb_win + pl.W - 1) // pl.W):
        idx = np.full((pl.W, pl.nb_win), INF)
        w = np.arange(pl.W)
        j = w + k * pl.W
        ok = j < pl.nb_win
        idx[w[ok], j[ok]] = rnd.randint(0, 2 * SK.POOL, size=int(ok.sum()))
        rep = rnd.randint(0, NREP, size=idx.shape)
        arrays, fold = run_all(probe, g, pl, n, c, tbl, glv, subs, gather(g, idx, rep).reshape(-1, g.PW), **knobs)
        done += check_all(g, pl, arrays, fold, logs_of(g, idx), "%s %r one-hot run %d" % (g.name, call, k))
    return done


# ---- what the tests sweep ----------------------------------------------------------------------------------------------------------

G1 = GROUPS[:4]
SERIAL_EDGES = [(K, 0, woff, n_old) for K in (2, 4, 8) for woff in (0, 1) for n_old in (0, 1, 2)]
COOP_EDGES = ([(K, 1, woff, n_old) for K in (16, 32, 64, 128, 256) for woff in (0, 1) for n_old in (0, 1, 5, 9, 14)] +
              [(K, 2, woff, n_old) for K in (16, 32, 64, 128) for woff in (0, 1) for n_old in (0, 1, 5, 9, 14)])
LARGE_N_OLD = 9                        # tuples from here up may run on one 12-limb and one 8-limb curve only
LARGE_N_OLD_GROUPS = ("bls12_381", "bn254", "bls12_381_g2")


def sweep_calls(g):
    """(n, c, tbl, glv, subs) of every plan whose levels the level tests run"""
    if g.g2:
        return [(n, c, 0, 0, 0) for c in (4, 7, 10, 13, 16) for n in (5000, 1 << 20)]
    calls = [(n, c, 0, 0, 0) for c in range(2, 21) for n in (5000, 1 << 20)]
    calls += [(n, c, 1, glv, 0) for c in (8, 13, 16, 20, 22, 23) for glv in (0, 1) for n in (5000, 1 << 20)]
    calls += [(rows * 1024, c, 1, glv, rows) for rows in (4, 8, 1024, 8192) for c in (8, 11, 13) for glv in (0, 1)]
    return calls


def level_tuples(probe, g):
    """the (K, mode, weight_off, n_old) of every level of every swept plan, and the fixed edges, without duplicates"""
    seen = set()
    for n, c, tbl, glv, subs in sweep_calls(g):
        pl = probe_plan(probe, g, n, c, tbl, glv, subs)
        assert pl != BAD_OP, (g.name, n, c, tbl, glv, subs)
        seen.update(pl.tuples())
    seen.update(SERIAL_EDGES)
    seen.update(t for t in COOP_EDGES if not (g.g2 and (t[1] == 2 or t[0] > 128)))
    return sorted(t for t in seen if t[3] < LARGE_N_OLD or g.name in LARGE_N_OLD_GROUPS)


def contents_for(g):
    return [c for c in CONTENTS if c != "lazy" or g.lazy_store]


# ---- whole MSMs with every bucket full ---------------------------------------------------------------------------------------------

def full_bucket_scalars(r, bits, c, limit=None):
    """one scalar per (window w, bucket j): (j + 1) 2^(c w), wherever that is below r (and below `limit`).  The recoding keeps digits
    up to 2^(c-1) positive, so every bucket receives exactly one base and none is cut; asserted with sortref's digits, not trusted"""
    windows, half = bits // c + 1, 1 << (c - 1)
    top = r if limit is None else min(r, limit)
    sc = [(j + 1) << (c * w) for w in range(windows) for j in range(half) if (j + 1) << (c * w) < top]
    d = S.recode(S.to_limbs(sc), c, windows)
    assert d.min() == 0 and d.max() == half and ((d != 0).sum(axis=1) == 1).all(), "a scalar has more than one digit"
    i, w = np.nonzero(d)
    keys = w * half + d[i, w] - 1
    assert len(np.unique(keys)) == len(sc), "two bases in one bucket"
    full = np.bincount(w, minlength=windows)
    assert (full[:(top.bit_length() - 1) // c] == half).all() and full.sum() == len(sc), "a window below the top one is not full"
    return sc


def choose_c(n, bits):
    """msm_choose_c (csrc/msm.hpp) restated: the width a table-free call of n pairs runs at"""
    if n < 32:
        return 3
    lg = n.bit_length() - 1
    c = min(max(lg - 4 if lg > 4 else 2, 4), 20)
    if n >= 1 << 16:
        for d in range(4):
            for cc in (c - d, c + d):
                if 8 <= cc <= 20 and bits - (bits // cc) * cc >= 7:
                    return cc
    return c
