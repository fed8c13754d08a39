"""streaming_kzg over Python integers, twice.

(A) the streaming algorithms as the reference runs them (poly-commit/src/streaming_kzg): coefficients arrive HIGHEST degree first,
    the key is the reversed vector of powers, the folding tree comes out of a stack iterator, the division keeps a deque of k
    values.  A restatement, statement by statement, of data_structures.rs:68-138 and space.rs:65-262.
(B) the array definitions the device computes (include/pc_hip.h): natural order (index = degree), one level after the other, long
    division by the vanishing polynomial.

The group side is the trapdoor: a key point is its exponent tau^d, an MSM is a dot product mod r, and the point is exponent * G
(`point`, pyref's curve arithmetic).  tests/test_skzg_cpu.py proves (A) == (B); the GPU tests compare the device with both."""
from collections import deque

import pyref as R


def ceil_div(a, b):
    return (a + b - 1) // b


def vanishing_polynomial(points, p):
    """prod (x - z_j), coefficients lowest degree first (mod.rs:279-285)"""
    z = [1]
    for pt in points:
        nxt = [0] * (len(z) + 1)
        for i, c in enumerate(z):
            nxt[i] = (nxt[i] - pt * c) % p
            nxt[i + 1] = (nxt[i + 1] + c) % p
        z = nxt
    return z


def evaluate_le(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def evaluate_be(coeffs, x, p):
    acc = 0
    for c in coeffs:
        acc = (acc * x + c) % p
    return acc


def powers(x, n, p):
    out = [1] * n
    for i in range(1, n):
        out[i] = x * out[i - 1] % p
    return out


def point(curve, exponent, G=None):
    """exponent * G as pyref's affine point (None = infinity)"""
    return R.ec_mul(curve, exponent, R.generator(curve) if G is None else G)


# ---- (A) the reference's streams --------------------------------------------------------------------------------------------

def init_stack(n, challenges_len):
    stack = []
    chunk_size = 1 << challenges_len
    if n % chunk_size != 0:
        delta = chunk_size - n % chunk_size
        for i in reversed(range(challenges_len)):
            if delta >= 1 << i:
                stack.append((i, 0))
                delta -= 1 << i
    return stack


class FoldedPolynomialTreeIter:
    """data_structures.rs:103-138 over a stream of coefficients, highest degree first"""

    def __init__(self, stream, n, challenges, p):
        self.challenges, self.iterator, self.p = challenges, iter(stream), p
        self.stack = init_stack(n, len(challenges))

    def __iter__(self):
        return self

    def __next__(self):
        while True:
            ln = len(self.stack)
            if ln > 1 and self.stack[ln - 1][0] == self.stack[ln - 2][0]:
                _level, lhs = self.stack[ln - 1]
                level, rhs = self.stack[ln - 2]
                del self.stack[ln - 2:]
                item = (level + 1, (rhs * self.challenges[level] + lhs) % self.p)
            else:
                item = (0, next(self.iterator))            # StopIteration ends the tree, as `?` does
            if item[0] != len(self.challenges):
                self.stack.append(item)
            if item[0] != 0:                               # the base polynomial is skipped
                return item


def reversed_key(tau, length, p):
    """CommitterKeyStream::from(&CommitterKey): Reverse(powers_of_g) -- stream position t holds tau^(length - 1 - t)"""
    return list(reversed(powers(tau, length, p)))


def space_open(key, stream, alpha, p):
    """space.rs:65-95: (evaluation, proof exponent)"""
    bases = iter(key[len(key) - len(stream):])
    previous, quotient = 0, 0
    for scalar, base in zip(stream, bases):
        quotient = (quotient + base * previous) % p
        previous = (previous * alpha + scalar) % p
    return previous, quotient


def space_open_multi_points(key, stream, points, p):
    """space.rs:98-136: (remainder as the deque leaves it, proof exponent)"""
    zeros = vanishing_polynomial(points, p)
    deg = len(zeros) - 1
    bases = iter(key[len(key) - len(stream) + deg:])
    it = iter(stream)
    state = deque(next(it) for _ in range(len(points)))
    quotient = 0
    for coefficient in it:
        quotient_coefficient = state.popleft()
        state.append(coefficient)
        for i in range(len(points)):
            state[i] = (state[i] - zeros[deg - i - 1] * quotient_coefficient) % p
        quotient = (quotient + next(bases) * quotient_coefficient) % p
    return list(state), quotient


def space_commit_folding(key, stream, challenges, p):
    """space.rs:165-199: the exponents of the commitments of the levels 1 .. depth"""
    n = len(challenges)
    sums, folded_bases = [0] * n, []
    for i in range(1, n + 1):
        delta = len(key) - ceil_div(len(stream), 1 << i)
        folded_bases.append(iter(key[delta:]))
    for i, coefficient in FoldedPolynomialTreeIter(stream, len(stream), challenges, p):
        sums[i - 1] = (sums[i - 1] + next(folded_bases[i - 1]) * coefficient) % p
    return sums


def space_open_folding(key, stream, challenges, points, etas, p):
    """space.rs:205-262: (remainders per level, proof exponent)"""
    n = len(challenges)
    zeros = vanishing_polynomial(points, p)
    deg = len(zeros) - 1
    remainders, folded_bases, acc = [], [], 0
    for i in range(1, n + 1):
        delta = len(key) - ceil_div(len(stream), 1 << i)
        remainders.append(deque([0] * len(points)))
        folded_bases.append(iter(key[delta:]))
    for i, coefficient in FoldedPolynomialTreeIter(stream, len(stream), challenges, p):
        if i == 0:
            continue
        base = next(folded_bases[i - 1])
        quotient_coefficient = remainders[i - 1].popleft()
        remainders[i - 1].append(coefficient)
        for j in range(len(points)):
            remainders[i - 1][j] = (remainders[i - 1][j] - zeros[deg - j - 1] * quotient_coefficient) % p
        acc = (acc + base * (etas[i - 1] * quotient_coefficient % p)) % p
    return [list(r) for r in remainders], acc


# ---- (B) the array definitions ----------------------------------------------------------------------------------------------

def fold_tree(f, challenges, p):
    """levels f_1 .. f_depth, lowest degree first"""
    levels, cur = [], list(f)
    for rho in challenges:
        nxt = [(cur[2 * b] + (rho * cur[2 * b + 1] if 2 * b + 1 < len(cur) else 0)) % p for b in range(ceil_div(len(cur), 2))]
        levels.append(nxt)
        cur = nxt
    return levels


def div_multi(f, points, p):
    """(q lowest degree first with max(n - k, 0) coefficients, r with k coefficients HIGHEST degree first)"""
    k, n = len(points), len(f)
    zeros = vanishing_polynomial(points, p)                # monic, degree k
    rem = list(f)
    q = [0] * max(n - k, 0)
    for d in reversed(range(len(q))):
        c = rem[d + k]
        q[d] = c
        for i in range(k + 1):
            rem[d + i] = (rem[d + i] - c * zeros[i]) % p
    r = (rem[:k] + [0] * k)[:k]
    return q, list(reversed(r))


def msm_exponent(scalars, tau, p, first=0):
    return sum(s * pow(tau, first + d, p) for d, s in enumerate(scalars)) % p


def open_multi(f, points, tau, p):
    q, r = div_multi(f, points, p)
    return r, msm_exponent(q, tau, p)


def batch_open_multi(polys, points, eta, tau, p):
    n = max(len(f) for f in polys)
    comb = [0] * n
    for e, f in zip(powers(eta, len(polys), p), polys):
        for i, c in enumerate(f):
            comb[i] = (comb[i] + e * c) % p
    return msm_exponent(div_multi(comb, points, p)[0], tau, p)


def commit_folding(f, challenges, tau, p):
    return [msm_exponent(lv, tau, p) for lv in fold_tree(f, challenges, p)]


def open_folding(f, challenges, points, etas, tau, p):
    rems, acc = [], 0
    for eta, lv in zip(etas, fold_tree(f, challenges, p)):
        q, r = div_multi(lv, points, p)
        rems.append(r)
        acc = (acc + eta * msm_exponent(q, tau, p)) % p
    return rems, acc
