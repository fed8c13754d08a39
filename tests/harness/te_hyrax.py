"""HyraxPC over ed_on_bls12_381 in pure Python: a restatement of poly-commit/src/hyrax/mod.rs:119-168 (setup) and :193-511 (commit,
open, check) for ONE polynomial over the group law of teref.py, with te_setup.py for the generators -- the checker of
poly_commit_amd/te_hyrax.py.  The reference's tests run this scheme on this curve and no other (Hyrax381, hyrax/tests.rs:6,20-21).

Field elements are canonical Python integers modulo teref.R, points (x, y) tuples.  The sponge is the caller's, as in hyrax.py: the
challenge c and the prover's random field elements are arguments, in the order the reference draws them.
"""
from . import te_setup as S
from . import teref as E

PROTOCOL_NAME = b"Hyrax protocol"      # hyrax/mod.rs:26
R = E.R


class InvalidNumberOfVariables(ValueError):
    """hyrax Error::InvalidNumberOfVariables"""


class IncorrectCommitmentSize(ValueError):
    """hyrax Error::IncorrectCommitmentSize"""


def setup(num_vars):
    """:119-168: dim + 1 generators of PROTOCOL_NAME from index 0 (the sampling loop is InnerProductArgPC's, te_setup.py); the last
    one is popped as h (:165)"""
    if num_vars is None or num_vars % 2 == 1:                      # :124-134
        raise InvalidNumberOfVariables(num_vars)
    dim = 1 << (num_vars // 2)                                     # :138
    pts, _ = S.generators(PROTOCOL_NAME, 0, dim + 1)               # :143-163
    return dict(com_key=pts[:dim], h=pts[dim])                     # :165-167


def trim(pp):
    """:176-183: a clone"""
    return pp, pp


def tensor_prime(values):
    """hyrax/utils.rs:27-39"""
    out = [1]
    for val in reversed(values):
        out = [v * (1 - val) % R for v in out] + [v * val % R for v in out]
    return out


def tensors(point):
    n = len(point)
    point_rev = list(reversed(point))                              # :299
    return tensor_prime(point_rev[n // 2:]), tensor_prime(point_rev[:n // 2])      # l, r: :301-307


def pedersen_commit(key, scalars):
    """:86-93; panics unless the lengths agree"""
    assert len(key) == len(scalars)
    return E.msm(key, scalars)


def evaluate(evals, point):
    """DenseMultilinearExtension::evaluate, directly: variable j is bit j of the index (little-endian)"""
    cur = [v % R for v in evals]
    assert len(cur) == 1 << len(point)
    for p in point:
        cur = [(cur[2 * i] * (1 - p) + cur[2 * i + 1] * p) % R for i in range(len(cur) // 2)]
    return cur[0]


def commit(ck, evals, rands):
    """:213-252 for one polynomial given by its evaluations; rands: the dim row randomisers, in row order.
    Returns (row_coms, state = (rands, the matrix as a list of rows))."""
    total = len(evals)
    n = total.bit_length() - 1
    assert total == 1 << n
    dim = 1 << (n // 2)                                            # :218
    if n % 2 == 1 or n > len(ck["com_key"]):                       # :220-228
        raise InvalidNumberOfVariables(n)
    # flat_to_matrix_column_major (hyrax/utils.rs:13-21): row r = flat[r], flat[dim + r], ...
    mat = [[evals[c * dim + r] % R for c in range(dim)] for r in range(dim)]       # :230
    assert len(rands) == dim
    row_coms = [E.add(pedersen_commit(ck["com_key"][:dim], row), E.mul(rr % R, ck["h"])) for row, rr in zip(mat, rands)]      # :233-242
    return row_coms, ([rr % R for rr in rands], mat)


def open(ck, state, point, r_eval, d, r_d, r_b, c):   # noqa: A001 (the reference's name)
    """:287-402; r_eval, d (dim elements), r_d, r_b: the random elements in the order they are drawn (:360, :367-368, :373, :377);
    c: the challenge (:389).  Returns ((com_eval, com_d, com_b, z, z_d, z_b), eval)."""
    n = len(point)
    if n % 2 == 1:                                                 # :289-293
        raise InvalidNumberOfVariables(n)
    dim = 1 << (n // 2)
    rands, mat = state
    assert len(mat) == dim                                         # :328-333 (MismatchedNumVars)
    l, r = tensors(point)
    g0, h = ck["com_key"][0], ck["h"]
    lt = [sum(l[i] * mat[i][j] for i in range(dim)) % R for j in range(dim)]       # :347, t.row_mul(l)
    r_lt = sum(a * b for a, b in zip(l, rands)) % R                                # :351-354
    ev = sum(a * b for a, b in zip(lt, r)) % R                                     # :356
    com_eval = E.add(E.mul(ev, g0), E.mul(r_eval % R, h))                          # :361
    assert len(d) == dim
    b = sum(a * x for a, x in zip(r, d)) % R                                       # :370
    com_d = E.add(pedersen_commit(ck["com_key"][:dim], [x % R for x in d]), E.mul(r_d % R, h))      # :374
    com_b = E.add(E.mul(b, g0), E.mul(r_b % R, h))                                 # :378
    z = [(x + c * y) % R for x, y in zip(d, lt)]                                   # :391
    z_d = (c * r_lt + r_d) % R                                                     # :392
    z_b = (c * r_eval + r_b) % R                                                   # :393
    return (com_eval, com_d, com_b, z, z_d, z_b), ev


def check(vk, row_coms, point, proof, c):
    """:430-511 for one commitment.  Returns bool."""
    n = len(point)
    if n % 2 == 1:                                                 # :432-436
        raise InvalidNumberOfVariables(n)
    dim = 1 << (n // 2)
    com_eval, com_d, com_b, z, z_d, z_b = proof
    if len(row_coms) != dim:                                       # :463-468
        raise IncorrectCommitmentSize((len(row_coms), dim))
    l, r = tensors(point)
    g0, h = vk["com_key"][0], vk["h"]
    ip = sum(a * x for a, x in zip(r, z)) % R
    com_dp = E.add(E.mul(ip, g0), E.mul(z_b % R, h))               # :492
    if com_dp != E.add(E.mul(c % R, com_eval), com_b):             # :493-495
        return False
    t_prime = E.msm(row_coms, l)                                   # :498-501
    com_z_zd = E.add(pedersen_commit(vk["com_key"][:dim], [x % R for x in z]), E.mul(z_d % R, h))      # :504
    return com_z_zd == E.add(E.mul(c % R, t_prime), com_d)         # :505-507
