"""The IPA of BLS12-377 through discrete logarithms: a checker that stays in seconds.

Pure-Python point arithmetic on a 377-bit field costs milliseconds per scalar multiplication, so the keys of these tests are
P_i = d_i G with known d_i: every group element the prover returns is then ONE computation in Fr plus one `B.mul_g`.

  ipa_rounds_dlog     `ipa_rounds` of the Python reference (oracle/pyref.py) restated over the logarithms of the key
  device_key          a device key with arbitrary logarithms (pc_hip_fixed_base_batch_mul on the log vector), and its check
  fold_case           a key of 2 * half points whose fold by u is an arithmetic progression e_0 + i delta of logarithms: the
                      expected key is a running chain of Python additions, one per point (points_of_logs)
  glv_constants / glv_split / longest_split
                      the GLV decomposition csrc/glv.hpp performs, from the generated constants, in Python integers
"""
import os
import random
import re

import numpy as np

from . import ref377 as B

R, CURVE, FR, r = B.R, B.CURVE, B.FR, B.RMOD
CSRC = os.path.join(B.ROOT, "poly_commit_amd", "csrc")


# ---- the halving rounds over logarithms ---------------------------------------------------------------------------------------------

def ipa_rounds_dlog(d, h_log, coeffs, z, challenges, p=r):
    """ipa_rounds (ipa_pc/mod.rs:664-711) for the key P_i = d[i] G and h' = h_log G: the logarithms of every L_j and R_j, the logarithm
    of the final key, and the final coefficient."""
    n = len(coeffs)
    assert n == len(d) and n & (n - 1) == 0
    key, cs = [x % p for x in d], [c % p for c in coeffs]
    zs = [1] * n
    for i in range(1, n):
        zs[i] = zs[i - 1] * z % p
    l_logs, r_logs = [], []
    for u in challenges[:n.bit_length() - 1]:
        h = n // 2
        ip_l = sum(a * b for a, b in zip(cs[h:n], zs[:h])) % p
        ip_r = sum(a * b for a, b in zip(cs[:h], zs[h:n])) % p
        l_logs.append((sum(k * c for k, c in zip(key[:h], cs[h:n])) + ip_l * h_log) % p)
        r_logs.append((sum(k * c for k, c in zip(key[h:n], cs[:h])) + ip_r * h_log) % p)
        ui = pow(u, -1, p)
        for i in range(h):
            cs[i] = (cs[i] + ui * cs[h + i]) % p
            zs[i] = (zs[i] + u * zs[h + i]) % p
            key[i] = (key[i] + u * key[h + i]) % p
        n = h
    return l_logs, r_logs, key[0], cs[0]


def log_points(logs):
    """words of d G for every logarithm (one mul_g each: for the handful of points a proof holds)"""
    return B.points([B.mul_g(d) if d % r else None for d in logs])


# ---- device keys with known logarithms ----------------------------------------------------------------------------------------------

def dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def filled(shape, value=-1):
    """a device tensor filled by torch, FINISHED: the library's streams do not wait for torch's, so a fill or a copy that torch has only
    queued could land after the library's kernel has written"""
    import torch
    t = torch.full(shape, value, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def copy_of(t):
    import torch
    c = t.clone()
    torch.cuda.synchronize()
    return c


def device_points(ctx, dlogs):
    """(n, 12) uint64 words of d_i G made on the device by pc_hip_fixed_base_batch_mul; d_i = 0 gives the all-zero infinity"""
    import torch
    n = len(dlogs)
    out = torch.empty((n, 12), dtype=torch.int64, device="cuda")
    sc = dev(B.fr_mont(dlogs))
    ctx.fixed_base_batch_mul(CURVE, B.point(B.G), sc.data_ptr(), n, out.data_ptr())
    return out.cpu().numpy().view(np.uint64)


def check_positions(dlogs):
    """the positions whose points are checked against mul_g: first, last, two interior ones -- and every d = 0"""
    n = len(dlogs)
    return sorted({0, n // 3, (2 * n) // 3, n - 1}), [i for i, d in enumerate(dlogs) if d % r == 0]


def check_key(words, dlogs):
    some, zeros = check_positions(dlogs)
    for i in some:
        assert (words[i] == B.point(B.mul_g(dlogs[i]) if dlogs[i] % r else None)).all(), i
    for i in zeros:
        assert not words[i].any(), i
    assert words.shape == (len(dlogs), 12)


def device_key(ctx, dlogs):
    """the checked words of the key d_i G (the caller uploads them, or a slice of them)"""
    words = device_points(ctx, dlogs)
    check_key(words, dlogs)
    return words


# ---- a fold whose expected result is an addition chain ------------------------------------------------------------------------------

def points_of_logs(logs, delta):
    """the points log_i G of a list of logarithms that is the arithmetic progression log_0 + i delta except at a few places: one
    Python addition per point where the step is delta, one mul_g where it is not"""
    step = B.mul_g(delta) if delta % r else None
    out, prev = [], None
    for e in logs:
        e %= r
        if prev is not None and (prev + delta) % r == e:
            A = R.ec_add(CURVE, out[-1], step)
        else:
            A = B.mul_g(e) if e else None
        out.append(A)
        prev = e
    return out


SPECIAL_LANES = ("kl_inf", "kr_inf", "both_inf", "doubling", "cancel")


def fold_case(half, u, seed, specials=None, inf_lo=None, inf_hi=None):
    """(dlogs of the 2 * half key points, expected points of the fold K_l[i] + u K_r[i], their logarithms, delta).

    Ordinary lanes: d_hi[i] random, d_lo[i] = e_0 + i delta - u d_hi[i], so the results are the chain e_0 G, (e_0 + delta) G, ...
    specials: {lane: kind} with kind in SPECIAL_LANES -- K_l at infinity, K_r at infinity, both, u K_r = K_l (the closing addition is
    a doubling), u K_r = -K_l (the result is the point at infinity); their expected points come from mul_g of the logarithm."""
    rnd = random.Random(seed)
    e0, delta = rnd.randrange(1, r), rnd.randrange(1, r)
    d_hi = R.gen_scalars(FR, seed, half)
    d_lo = [(e0 + i * delta - u * d_hi[i]) % r for i in range(half)]
    specials = dict(specials or {})
    if inf_lo is not None:
        specials[inf_lo] = "kl_inf"
    if inf_hi is not None:
        specials[inf_hi] = "kr_inf"
    for i, kind in specials.items():
        assert kind in SPECIAL_LANES
        if kind in ("kl_inf", "both_inf"):
            d_lo[i] = 0
        if kind in ("kr_inf", "both_inf"):
            d_hi[i] = 0
        if kind == "doubling":
            d_lo[i] = u * d_hi[i] % r
        if kind == "cancel":
            d_lo[i] = -u * d_hi[i] % r
    e = [(a + u * b) % r for a, b in zip(d_lo, d_hi)]
    return d_lo + d_hi, points_of_logs(e, delta), e, delta


# ---- GLV in Python integers ---------------------------------------------------------------------------------------------------------

def _struct(header, name):
    src = open(os.path.join(CSRC, header)).read()
    i = src.index("struct %s {" % name)
    return src[i:src.index("\n};", i)]


def _words(body, field):
    m = re.search(r"\b%s\[\d+\]\s*=\s*\{([^}]*)\}" % field, body)
    w = [int(x.strip().rstrip("ul"), 16) for x in m.group(1).split(",")]
    bits = 64 if "ull" in m.group(1) else 32
    return sum(v << (bits * i) for i, v in enumerate(w))


def glv_constants(curve=CURVE):
    """lambda, the lattice basis (signed) and the rounding constants of pc_glv_<curve> (csrc/glv_constants.h)"""
    body = _struct("glv_constants.h", "pc_glv_" + curve)
    flag = lambda f: int(re.search(r"\b%s = (\d+)" % f, body).group(1))            # noqa: E731
    sg = lambda f: -_words(body, f) if flag(f + "_NEG") else _words(body, f)        # noqa: E731
    return dict(lam=_words(body, "LAMBDA"), a1=sg("A1"), b1=sg("B1"), a2=sg("A2"), b2=sg("B2"), g1=_words(body, "G1"), g2=_words(body, "G2"),
                n1neg=flag("N1_NEG"), n2neg=flag("N2_NEG"))


def glv_split(k, g=None):
    """(k1, k2) signed with k = k1 + k2 lambda (mod r): glv_decompose of csrc/glv.hpp (Babai rounding with truncated quotients)"""
    g = g or glv_constants()
    c1, c2 = (g["g1"] * k) >> 384, (g["g2"] * k) >> 384
    c1, c2 = (-c1 if g["n1neg"] else c1), (-c2 if g["n2neg"] else c2)
    return k - c1 * g["a1"] - c2 * g["a2"], -c1 * g["b1"] - c2 * g["b2"]


LONGEST_SEED, LONGEST_TRIES = 0x377617, 4000


def seeded_challenges(p=r):
    """the LONGEST_TRIES seeded values the search below runs over"""
    rnd = random.Random(LONGEST_SEED)
    return [rnd.randrange(p) for _ in range(LONGEST_TRIES)]


def longest_split(p=r, g=None):
    """(challenge, bit length of its longer half): the seeded value, of LONGEST_TRIES, whose split has the largest max(|k1|, |k2|)"""
    g = g or glv_constants()
    best, best_k = -1, None
    for k in seeded_challenges(p):
        m = max(abs(x) for x in glv_split(k, g))
        if m > best:
            best, best_k = m, k
    return best_k, best.bit_length()


def edge_challenges(p=r, curve=CURVE):
    """(name, challenge) at which a GLV split or a NAF recoding can go wrong, and one random value"""
    g = glv_constants(curve)
    lam = g["lam"]
    worst, _ = longest_split(p, g)
    return [("0", 0), ("1", 1), ("2", 2), ("r-1", p - 1), ("lambda", lam), ("r-lambda", p - lam), ("lambda+1", lam + 1), ("lambda-1", lam - 1),
            ("2^252", (1 << 252) % p), ("random", random.Random(0xC4A11E).randrange(p)), ("longest split", worst)]
