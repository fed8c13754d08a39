"""MarlinPST13 over Python integers, twice.

(A) the reference's algorithms on term dictionaries (poly-commit/src/marlin/marlin_pst13_pc/mod.rs): a polynomial is a dict
    {exponent tuple of length n: coefficient}; `divide_at_point` follows mod.rs:44-92 term by term and, as the reference does, DROPS
    constant terms; `commit` and `open` are the sums over terms of mod.rs:353-362 and :457-469 in the exponent of G (the key is
    known through its trapdoor: the point of the term e is (prod_j beta_j^e_j) G).
(B) the dense definitions of include/pc_hip.h: the lexicographic layout (`rank`, `unrank`, `key_len`), the dense vector of a
    polynomial, and the division along one variable fiber by fiber (`dense_divide`), which keeps the constants: its last remainder
    is p(z).

tests/test_pst13_cpu.py proves (A) == (B) once constants are set aside; the GPU tests compare the device with both."""
from math import comb


# ---- (B) the layout ---------------------------------------------------------------------------------------------------------------

def N(v, r):
    """monomials in v variables of total degree <= r"""
    return comb(v + r, v) if r >= 0 else 0


def key_len(n, d):
    return N(n, d)


def rank(e, d):
    """the formula of the issue / pc_hip.h: v_j = n - j - 1 variables after j, r_j = d - (e_0 + .. + e_{j-1})"""
    n, r, k = len(e), d, 0
    for j, ej in enumerate(e):
        v = n - j - 1
        k += comb(v + r + 1, v + 1) - comb(v + r - ej + 1, v + 1)
        r -= ej
    assert r >= 0, "degree above the layout's"
    return k


def monomials(n, d):
    """every exponent tuple of degree <= d in tuple (lexicographic) order"""
    if n == 0:
        return [()]
    return [(e0,) + t for e0 in range(d + 1) for t in monomials(n - 1, d - e0)]


def unrank(k, n, d):
    e, r = [], d
    for j in range(n):
        v = n - j - 1
        ej = 0
        while ej < r and comb(v + r + 1, v + 1) - comb(v + r - ej, v + 1) <= k:
            ej += 1
        k -= comb(v + r + 1, v + 1) - comb(v + r - ej + 1, v + 1)
        r -= ej
        e.append(ej)
    return tuple(e)


def to_dense(terms, n, d, p):
    """terms: dict or list of (exps, coeff); like terms are merged (from_coefficients_vec)"""
    out = [0] * key_len(n, d)
    for e, c in (terms.items() if isinstance(terms, dict) else terms):
        out[rank(e, d)] = (out[rank(e, d)] + c) % p
    return out


def from_dense(vec, n, d):
    return {unrank(k, n, d): c for k, c in enumerate(vec) if c}


def dense_divide(vec, n, d, z, p):
    """the n passes: returns ([w_0 .. w_{n-1}], p(z)); w_i is a dense vector of N(n - i, d) slots in the layout (n - i, d)"""
    cur, quotients = list(vec), []
    for i in range(n):
        nv = n - i
        q, rem = [0] * N(nv, d), [0] * N(nv - 1, d)
        slot_of = {e: k for k, e in enumerate(monomials(nv, d))}  # == rank(e, d): the tuple order (test_pst13_cpu.py), looked up
        for f, tail in enumerate(monomials(nv - 1, d)):           # fiber f: the tail of rank f
            acc = 0                                               # q[d - s] = 0
            for k in range(d - sum(tail), -1, -1):
                slot = slot_of[(k,) + tail]
                q[slot] = acc
                acc = (cur[slot] + z[i] * acc) % p
            rem[f] = acc
        quotients.append(q)
        cur = rem
    return quotients, cur[0]


# ---- (A) the reference on term dictionaries -------------------------------------------------------------------------------------

def from_coefficients_vec(terms, p):
    """SparsePolynomial::from_coefficients_vec: like terms merged, zero coefficients dropped"""
    out = {}
    for c, e in terms:
        out[e] = (out.get(e, 0) + c) % p
    return {e: c for e, c in out.items() if c}


def evaluate(poly, point, p):
    acc = 0
    for e, c in poly.items():
        for x, ej in zip(point, e):
            c = c * pow(x, ej, p) % p
        acc = (acc + c) % p
    return acc


def degree(poly):
    return max((sum(e) for e in poly), default=0)


def divide_at_point(poly, point, n, p):
    """mod.rs:44-92"""
    if not poly:
        return [{} for _ in range(n)]
    quotients, cur = [], dict(poly)
    for i in range(n):
        quotient_terms, remainder_terms = [], []
        for e, coeff in cur.items():
            if not any(e):                                        # constants cancel out (:60-64)
                continue
            t = list(e)
            if t[i]:
                while t[i] > 1:                                   # :72-78
                    t[i] -= 1
                    quotient_terms.append((coeff, tuple(t)))
                    coeff = coeff * point[i] % p
                t[i] = 0                                          # :80-82
                quotient_terms.append((coeff, tuple(t)))
                remainder_terms.append((point[i] * coeff % p, tuple(t)))
            else:
                remainder_terms.append((coeff, e))
        quotients.append(from_coefficients_vec(quotient_terms, p))
        cur = from_coefficients_vec(remainder_terms, p)
    return quotients


def commit_exponent(poly, betas, p):
    """mod.rs:353-362 through the trapdoor: the commitment is (sum_terms c * prod_j beta_j^e_j) G = p(beta) G"""
    return evaluate(poly, betas, p)


def open_exponents(poly, point, betas, n, p):
    """mod.rs:457-469: the exponent of every w_i"""
    return [evaluate(w, betas, p) for w in divide_at_point(poly, point, n, p)]


def check_identity(poly, point, n, at, p):
    """mod.rs:41 evaluated at `at`: p(at) - p(z) == sum_i (at_i - z_i) w_i(at)"""
    ws = divide_at_point(poly, point, n, p)
    rhs = sum((at[i] - point[i]) * evaluate(ws[i], at, p) for i in range(n)) % p
    return (evaluate(poly, at, p) - evaluate(poly, point, p)) % p == rhs


# ---- hiding (data_structures.rs: Randomness::rand is a sum of univariates; mod.rs:377-403, :474-506) -------------------------------

def blinding_terms(n, degree, coeffs):
    """the blinding polynomial from the mirror's coefficient order: the constant, then X_j^1 .. X_j^degree for j = 0 .. n-1
    (degree = hiding_bound + 1, calculate_hiding_polynomial_degree); coeffs: 1 + n degree values"""
    out = {(0,) * n: coeffs[0]}
    for j in range(n):
        for t in range(1, degree + 1):
            out[tuple(t if i == j else 0 for i in range(n))] = coeffs[1 + j * degree + t - 1]
    return out


def hiding_key_exponent(e, gamma, betas, p):
    """the hiding key's point of a univariate term: gamma * prod beta^e"""
    acc = gamma
    for x, ej in zip(betas, e):
        acc = acc * pow(x, ej, p) % p
    return acc
