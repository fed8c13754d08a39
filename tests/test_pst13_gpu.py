"""GPU suite of MarlinPST13 (pc_hip_pst13_monomial_evals, _scatter, _divide, _commit, _open, _trim and host/marlin_pst13.hpp)
against TRUE keys made by the new setup path from a known trapdoor: every field element bit for bit against the dense definitions
and the term-dictionary restatement of tests/harness/pst13.py, every group element through the trapdoor (a commitment or proof over
scalars s is (sum_r s[r] prod_j beta_j^e_j(r)) G).

Shapes (n, d): (1, 1), (2, 1) degenerate; (1, 5) the univariate route; (3, 4), (4, 3) the same M = 35 in two layouts; (5, 2) more
variables than degree; (3, 17) M = 1140, more than one workgroup, 171 fibers of lengths 1 .. 18 in pass 0; (6, 6) six passes;
(2, 255) M = 32896, the longest fiber."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref as R
from harness import pst13 as H

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (2, 1), (1, 5), (3, 4), (4, 3), (5, 2), (3, 17), (6, 6), (2, 255)]
CURVES = ["bls12_381", "bn254"]


class Cv:
    """what the tests need of a curve: Fr as Montgomery words, exponent -> affine Montgomery words"""

    def __init__(self, curve):
        self.curve = curve
        if curve == "bls12_377":
            from harness import ref377 as B
            self.p, self.mont, self.ints, self.limbs = B.RMOD, B.fr_mont, B.fr_from_mont, 6
            self.point = lambda k: B.point(B.mul_g(k) if k % B.RMOD else None)
        else:
            self.p, self.limbs = R.FIELDS[R.CURVES[curve]["fr"]]["p"], O.fq_limbs(curve)
            self.mont = lambda v: O.fr_mont_array(curve, list(v)) if len(v) else np.zeros((0, 4), dtype=np.uint64)
            self.ints = lambda a: O.fr_from_mont_array(curve, np.ascontiguousarray(a).reshape(-1, 4))
            g = R.gen_bases(curve, 1)[0]
            self.point = lambda k: O.points_to_array(curve, [R.ec_mul(curve, k % self.p, g) if k % self.p else None])[0]


@functools.lru_cache(maxsize=None)
def cv(curve):
    return Cv(curve)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def _betas(curve, n):
    rnd = random.Random("betas %s %d" % (curve, n))
    return [rnd.randrange(2, cv(curve).p) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _monomial_values(curve, n, d):
    """prod_j beta_j^e_j for every monomial in device order"""
    c, betas = cv(curve), _betas(curve, n)
    pw = [[pow(b, t, c.p) for t in range(d + 1)] for b in betas]
    out = []
    for e in H.monomials(n, d):
        acc = 1
        for j, ej in enumerate(e):
            acc = acc * pw[j][ej] % c.p
        out.append(acc)
    return out


_keys = {}


def make_key(ctx, curve, n, d):
    """setup's powers_of_g: monomial evaluations, then the fixed-base multiplication, into a resident key.  ONE key is alive at a
    time (a key brings three MSM pipelines with their queues and workspaces; making one takes milliseconds)"""
    import torch
    if (curve, n, d) not in _keys:
        _release_keys()
        c, M = cv(curve), H.key_len(n, d)
        ev = torch.full((M + 1, 4), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()      # torch's fill is only queued and the library's streams do not wait for torch's: finish it before the library writes
        ctx.pst13_monomial_evals(curve, n, d, c.mont(_betas(curve, n)), ev.data_ptr())
        pts = torch.empty((M, 2 * c.limbs), dtype=torch.int64, device="cuda")
        ctx.fixed_base_batch_mul(curve, c.point(1), ev.data_ptr(), M, pts.data_ptr())
        _keys[(curve, n, d)] = (ctx.upload_srs(curve, pts.data_ptr(), n=M), ev.cpu().numpy().view(np.uint64))
    return _keys[(curve, n, d)]


def _release_keys():
    for srs, _ in _keys.values():
        srs.free()
    _keys.clear()


@pytest.fixture(scope="module", autouse=True)
def _free_keys():
    yield
    _release_keys()


def polynomials(curve, n, d):
    """name -> term dictionary: all M terms random; the reference's `rand` shape (a sum of univariates); zero; constant only; the
    single term X_{n-1}^d; a few terms of which one has coefficient zero"""
    c = cv(curve)
    rnd = random.Random("polys %s %d %d" % (curve, n, d))
    mons = H.monomials(n, d)
    uni = {(0,) * n: rnd.randrange(c.p)}
    for j in range(n):
        for t in range(1, d + 1):
            uni[tuple(t if i == j else 0 for i in range(n))] = rnd.randrange(c.p)
    few = {e: rnd.randrange(1, c.p) for e in rnd.sample(mons, min(len(mons), 5))}
    few[next(iter(few))] = 0
    return {"full": {e: rnd.randrange(c.p) for e in mons}, "univariates": uni, "zero": {}, "constant": {(0,) * n: rnd.randrange(1, c.p)},
            "single": {(0,) * (n - 1) + (d,): rnd.randrange(1, c.p)}, "zero_coeff": few}


def points(curve, n):
    """random; one with a coordinate 0; one with all coordinates equal"""
    c = cv(curve)
    rnd = random.Random("points %s %d" % (curve, n))
    a, b = [rnd.randrange(c.p) for _ in range(n)], [rnd.randrange(c.p) for _ in range(n)]
    b[n // 2] = 0
    return {"random": a, "zero_coordinate": b, "equal": [a[0]] * n}


def cases(curve, n, d):
    """(polynomial, point) pairs, the same list for every shape: the full polynomial at every point, every other polynomial at one
    point each (all three kinds met)"""
    P, Z = polynomials(curve, n, d), points(curve, n)
    out = [("full", P["full"], z) for z in Z.values()]
    for (name, poly), z in zip([kv for kv in P.items() if kv[0] != "full"], list(Z.values()) * 2):
        out.append((name, poly, z))
    return out


def terms_arrays(curve, poly, n):
    exps = np.array(list(poly.keys()), dtype=np.uint8).reshape(-1, n)
    return exps, cv(curve).mont(list(poly.values()))


def dot(a, b, p):
    return sum(x * y for x, y in zip(a, b)) % p


# ---- setup ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_setup_monomial_evaluations_and_key_points(ctx, curve, n, d):
    c, M = cv(curve), H.key_len(n, d)
    srs, ev = make_key(ctx, curve, n, d)
    want = _monomial_values(curve, n, d)
    assert c.ints(ev[:M]) == want                                 # powers_of_beta in device order, bit for bit
    assert (ev[M] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the last rank"
    rnd = random.Random(n * 1000 + d)
    for r in sorted({0, 1, M - 1} | set(rnd.sample(range(M), min(M, 3)))):
        assert (srs.read(r, 1)[0] == c.point(want[r])).all(), (n, d, r)      # powers_of_g[rank(e)] == (prod beta^e) G


# ---- scatter ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_scatter(ctx, curve, n, d):
    import torch
    import poly_commit_amd._ffi as F
    c, M = cv(curve), H.key_len(n, d)
    for name, poly in polynomials(curve, n, d).items():
        exps, co = terms_arrays(curve, poly, n)
        want = c.mont(H.to_dense(poly, n, d, c.p))
        for on_device in (False, True):
            out = torch.full((M + 1, 4), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if on_device and len(poly):
                e_dev, c_dev = torch.from_numpy(exps.copy()).cuda(), _dev(co)
                ctx.pst13_scatter(curve, n, d, e_dev, c_dev, out.data_ptr(), n_terms=len(poly))
            else:
                ctx.pst13_scatter(curve, n, d, exps, co, out.data_ptr())
            got = out.cpu().numpy().view(np.uint64)
            assert (got[:M] == want).all(), (name, on_device)
            assert (got[M] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the vector"
    poly = polynomials(curve, n, d)["full"]
    exps, co = terms_arrays(curve, poly, n)
    out = torch.empty((M, 4), dtype=torch.int64, device="cuda")
    last = exps.shape[0] - 1
    for a, b in ((0, last), (last // 2, 0)):                      # the repeat after and before its twin
        e2 = np.vstack([exps, exps[a:a + 1]])
        for c2 in (np.vstack([co, co[b:b + 1]]) if last else np.vstack([co, c.mont([7])]), np.vstack([co, co[a:a + 1]])):      # different, then equal coefficients
            with pytest.raises(F.PcHipError) as err:
                ctx.pst13_scatter(curve, n, d, e2, c2, out.data_ptr())
            assert err.value.status == -1 and "repeated" in str(err.value)
    over = np.zeros((1, n), dtype=np.uint8)
    over[0, n - 1] = d                                            # degree d + 1 (an exponent is one byte: d = 255 takes two variables)
    over[0, 0] += 1
    with pytest.raises(F.PcHipError) as err:
        ctx.pst13_scatter(curve, n, d, np.vstack([exps, over]), np.vstack([co, co[:1]]), out.data_ptr())
    assert err.value.status == -1 and "degree" in str(err.value)


# ---- divide -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_divide(ctx, curve, n, d):
    import torch
    import poly_commit_amd._ffi as F
    c, M = cv(curve), H.key_len(n, d)
    prefix = [H.N(n - i, d) for i in range(n)]
    total = sum(prefix)
    for name, poly, z in cases(curve, n, d):
        vec = H.to_dense(poly, n, d, c.p)
        want, value = H.dense_divide(vec, n, d, z, c.p)
        src = c.mont(vec)
        for inp in (src, _dev(src)):
            quot = torch.full((total + 1, 4), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            offs, val = ctx.pst13_divide(curve, n, d, inp if isinstance(inp, np.ndarray) else inp.data_ptr(), c.mont(z), quot.data_ptr(), total)
            assert offs == [sum(prefix[:i]) for i in range(n)]   # the offsets are the prefix lengths, summed
            got = quot.cpu().numpy().view(np.uint64)
            assert (got[total] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "written past the last quotient"
            assert (got[:total] == c.mont([x for w in want for x in w])).all(), (name, n, d)      # every quotient slot, bit for bit
            assert c.ints(val) == [value] and value == H.evaluate(poly, z, c.p)
            if not isinstance(inp, np.ndarray):
                assert (inp.cpu().numpy().view(np.uint64) == src).all(), "the input vector is left unchanged"
        # the reference's own quotients (constants dropped on its way) are these
        if M <= 1200:                                             # (from_dense unranks every slot in Python: seconds at M = 32896)
            ref = H.divide_at_point(H.from_coefficients_vec([(co, e) for e, co in poly.items()], c.p), z, n, c.p)
            for i in range(n):
                assert {(0,) * i + e: x for e, x in H.from_dense(want[i], n - i, d).items()} == ref[i], (name, i)
    with pytest.raises(F.PcHipError):
        ctx.pst13_divide(curve, n, d, src, c.mont(z), quot.data_ptr(), total - 1)      # capacity below sum N(n - i, d)


# ---- commit and open --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_commit(ctx, curve, n, d):
    c = cv(curve)
    srs, _ = make_key(ctx, curve, n, d)
    mv, betas = _monomial_values(curve, n, d), _betas(curve, n)
    for name, poly in polynomials(curve, n, d).items():
        vec = H.to_dense(poly, n, d, c.p)
        exponent = dot(vec, mv, c.p)
        assert exponent == H.evaluate(poly, betas, c.p) == H.commit_exponent(poly, betas, c.p)      # p(beta), and the harness's sum over terms
        want = c.point(exponent)
        exps, co = terms_arrays(curve, poly, n)
        dense = c.mont(vec)
        for got, inf in (srs.pst13_commit(n, d, exps=exps, coeffs=co), srs.pst13_commit(n, d, dense=dense), srs.pst13_commit(n, d, dense=_dev(dense))):
            assert (got == want).all() and inf == (exponent == 0), (name, n, d)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_open(ctx, curve, n, d):
    c = cv(curve)
    srs, _ = make_key(ctx, curve, n, d)
    mv, betas = _monomial_values(curve, n, d), _betas(curve, n)
    prefix = [H.N(n - i, d) for i in range(n)]
    for k, (name, poly, z) in enumerate(cases(curve, n, d)):
        vec = H.to_dense(poly, n, d, c.p)
        ws, value = H.dense_divide(vec, n, d, z, c.p)
        # w_i lives on the prefix: its slot r is the monomial of rank r of the WHOLE key
        w_beta = [dot(ws[i], mv, c.p) for i in range(n)]
        # the trapdoor form of `check` (mod.rs:516-558 without the pairing): p(beta) - p(z) == sum_i (beta_i - z_i) w_i(beta)
        assert (dot(vec, mv, c.p) - value) % c.p == sum((betas[i] - z[i]) * w_beta[i] for i in range(n)) % c.p
        if H.key_len(n, d) <= 1200:
            assert w_beta == H.open_exponents(H.from_coefficients_vec([(co, e) for e, co in poly.items()], c.p), z, betas, n, c.p)
        if k % 2:
            exps, co = terms_arrays(curve, poly, n)
            got, inf, val = srs.pst13_open(n, d, c.mont(z), exps=exps, coeffs=co)
        else:
            got, inf, val = srs.pst13_open(n, d, c.mont(z), dense=_dev(c.mont(vec)))
        assert c.ints(val) == [value]
        for i in range(n):
            assert (got[i] == c.point(w_beta[i])).all() and inf[i] == (w_beta[i] == 0), (name, n, d, i)      # w_i == w_i(beta) G
        if name == "zero":
            assert inf.all() and not got.any()                   # n infinities
        univariate, pairs = ctx.last_pst13_shape()
        assert (univariate, pairs) == ((True, [d]) if n == 1 else (False, prefix)), "MSM i runs over the prefix N(n - i, d) only"


def test_a_key_of_another_length_or_offset_is_refused(ctx):
    import poly_commit_amd._ffi as F
    c = cv("bn254")
    srs, _ = make_key(ctx, "bn254", 3, 4)
    dense = c.mont([1] * 35)
    for call in (lambda: srs.pst13_commit(3, 5, dense=c.mont([1] * 56)), lambda: srs.pst13_commit(3, 4, dense=dense, base_offset=1),
                 lambda: srs.pst13_open(3, 4, c.mont([1, 2, 3]), dense=dense, base_offset=1), lambda: srs.pst13_trim(3, 5, 2)):
        with pytest.raises(F.PcHipError) as err:
            call()
        assert err.value.status == -1


def test_bls12_377_commit_and_open(ctx):
    curve, n, d = "bls12_377", 3, 4
    c = cv(curve)
    srs, ev = make_key(ctx, curve, n, d)
    mv, betas = _monomial_values(curve, n, d), _betas(curve, n)
    assert c.ints(ev[:35]) == mv and (srs.read(34, 1)[0] == c.point(mv[34])).all()
    poly, z = polynomials(curve, n, d)["full"], points(curve, n)["zero_coordinate"]
    vec = H.to_dense(poly, n, d, c.p)
    exps, co = terms_arrays(curve, poly, n)
    got, inf = srs.pst13_commit(n, d, exps=exps, coeffs=co)
    assert (got == c.point(dot(vec, mv, c.p))).all() and not inf
    ws, value = H.dense_divide(vec, n, d, z, c.p)
    got, inf, val = srs.pst13_open(n, d, c.mont(z), dense=c.mont(vec))
    assert c.ints(val) == [value] and not inf.any()
    for i in range(n):
        assert (got[i] == c.point(dot(ws[i], mv, c.p))).all(), i


@pytest.mark.parametrize("n,d", [(3, 4), (3, 17)])
def test_bls12_377_setup_scatter_and_divide(ctx, n, d):
    """pc_hip_pst13_monomial_evals, _scatter and _divide called directly for BLS12-377: the checks of the three tests above, every word,
    at M = 35 and at M = 1140 (more than one workgroup, fibers of lengths 1 .. 18)"""
    test_setup_monomial_evaluations_and_key_points(ctx, "bls12_377", n, d)
    test_scatter(ctx, "bls12_377", n, d)
    test_divide(ctx, "bls12_377", n, d)


def test_bls12_377_trim(ctx):
    """pc_hip_pst13_trim for BLS12-377, on a key whose points test_bls12_377_setup_scatter_and_divide compares with the trapdoor"""
    test_trim_is_the_key_of_the_smaller_degree(ctx, "bls12_377")


# ---- trim -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", CURVES)
def test_trim_is_the_key_of_the_smaller_degree(ctx, curve):
    big, _ = make_key(ctx, curve, 3, 4)
    for s in (1, 2, 4):
        small = big.pst13_trim(3, 4, s)
        try:
            want = [H.rank(e, 4) for e in H.monomials(3, s)]
            assert small.n == len(want)
            assert (small.read(0, small.n) == big.read(0, 35)[want]).all(), s
        finally:
            small.free()
    uni, _ = make_key(ctx, curve, 1, 5)                          # (releases `big`)
    small = uni.pst13_trim(1, 5, 2)
    assert (small.read(0, 3) == uni.read(0, 3)).all()
    small.free()


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

def _words(line):
    return [int(w, 16) for w in line.split()]


def test_host_mirror(ctx):
    """tests/cpp/pst13_driver.cpp prints its inputs and results; they are recomputed here: a two-polynomial open with given
    challenges without hiding, with hiding bound 1 and with hiding bound d - 1 (bound d is HidingBoundToolarge, checked in the driver,
    as are trim 4 -> 2 against a setup at 2 and PolynomialDegreeTooLarge); vk.beta_h against g2ref"""
    from harness import g2ref as G
    curve, n, d = "bls12_381", 3, 4
    c = cv(curve)
    exe = os.path.join(HERE, "cpp", "pst13_driver")
    root = os.path.dirname(HERE)
    srcs = [exe + ".cpp", os.path.join(root, "poly_commit_amd", "libpc_hip.so"), os.path.join(root, "include", "pc_hip.h")] + \
        [os.path.join(root, "poly_commit_amd", "host", f) for f in ("marlin_pst13.hpp", "kzg10.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in srcs):      # never a stale binary against a newer header
        libdir = os.path.join(os.path.dirname(HERE), "poly_commit_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, exe + ".cpp", "-L" + libdir, "-lpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    h = G.generator()
    h_words = np.frombuffer(G.point_bytes(h), dtype=np.uint64)
    r = subprocess.run([exe, " ".join("%x" % w for w in h_words)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "marlin_pst13 host mirror OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    head, runs, cur = {}, [], None
    for line in r.stdout.splitlines():
        if ":" not in line:
            continue
        name, _, rest = line.partition(":")
        if name == "case":
            cur = {"bound": int(rest)}
            runs.append(cur)
        elif name == "beta_h":
            head.setdefault("beta_h", []).append(_words(rest))
        else:
            (head if cur is None else cur)[name] = _words(rest)

    def fr(words):
        return c.ints(np.array(words, dtype=np.uint64).reshape(-1, 4))

    def pts(words):
        return np.array(words, dtype=np.uint64).reshape(-1, 2 * c.limbs)

    def poly(name):
        e = np.array(head[name + "_exps"], dtype=np.uint8).reshape(-1, n)
        return H.from_coefficients_vec([(co, tuple(int(x) for x in row)) for co, row in zip(fr(head[name + "_coeffs"]), e)], c.p)
    betas, gamma = fr(head["betas"]), fr(head["gamma"])[0]
    z, ch = fr(head["point"]), fr(head["challenges"])
    a, b = poly("a"), poly("b")
    for j, bh in enumerate(head["beta_h"]):                        # beta_h[j] = beta_j h (mod.rs:236)
        assert np.array(bh, dtype=np.uint64).tobytes() == G.point_bytes(G.mul(betas[j], h)), j
    assert len(head["beta_h"]) == n and [run["bound"] for run in runs] == [0, 1, d - 1]
    # setup's hiding key, every point against the oracle's ec_mul: [gamma G, then gamma beta_j^t G for t = 1 .. d + 1 per variable]
    hk = pts(head["hiding_key"])
    assert hk.shape[0] == 1 + n * (d + 1) and (hk[0] == c.point(gamma)).all()
    for j in range(n):
        for t in range(1, d + 2):
            assert (hk[1 + j * (d + 1) + t - 1] == c.point(gamma * pow(betas[j], t, c.p))).all(), (j, t)
    comb = H.from_coefficients_vec([(ch[0] * co, e) for e, co in a.items()] + [(ch[1] * co, e) for e, co in b.items()], c.p)
    w_plain = H.open_exponents(comb, z, betas, n, c.p)
    for run in runs:
        hb = run["bound"]
        blind = [{}, {}]
        if hb:
            blind = [H.blinding_terms(n, hb + 1, fr(run["blinding_" + x])) for x in "ab"]
        # commit: p(beta) G + r(beta) gamma G (mod.rs:353-403)
        for x, q, r_ in (("a", a, blind[0]), ("b", b, blind[1])):
            exponent = (H.evaluate(q, betas, c.p) + gamma * H.evaluate(r_, betas, c.p)) % c.p
            assert (pts(run["comm_" + x])[0] == c.point(exponent)).all(), (hb, x)
        # open: w_i = w_i(beta) G + (hiding witness i)(beta) gamma G (:457-506), random_v = r(z)
        rcomb = H.from_coefficients_vec([(ch[0] * co, e) for e, co in blind[0].items()] + [(ch[1] * co, e) for e, co in blind[1].items()], c.p)
        w_hide = H.open_exponents(rcomb, z, betas, n, c.p) if hb else [0] * n
        got = pts(run["w"])
        for i in range(n):
            assert (got[i] == c.point((w_plain[i] + gamma * w_hide[i]) % c.p)).all(), (hb, i)
        if hb:
            assert fr(run["random_v"]) == [H.evaluate(rcomb, z, c.p)]
            assert all(len(w) <= d for w in H.divide_at_point(rcomb, z, n, c.p)), "a hiding witness has at most d terms"
        else:
            assert "random_v" not in run
