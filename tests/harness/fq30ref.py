"""Python-integer side of the radix-2^30 form of BLS12-381 Fq (csrc/fp30.hpp): limb conversions, the boundary values of an operand
class and the exact value of its Montgomery product.  Shared by tests/test_fq30_cpu.py and the device probe tests."""
import numpy as np

import pyref as R

P = R.FIELDS["bls12_381_fq"]["p"]
W, N, MASK = 30, 13, (1 << 30) - 1
RP = 1 << (W * N)            # R' = 2^390
R32 = 1 << 384


def to13(v):
    """an integer as 13 limbs: limbs 0..11 of 30 bits, limb 12 the rest"""
    assert 0 <= v < 1 << (W * 12 + 32)
    return np.array([(v >> (W * i)) & MASK for i in range(12)] + [v >> (W * 12)], dtype=np.uint32)


def from13(a):
    return sum(int(x) << (W * i) for i, x in enumerate(a))


def to12(v):
    assert 0 <= v < R32
    return np.array([(v >> (32 * i)) & 0xffffffff for i in range(12)], dtype=np.uint32)


def from12(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def normalised(a):
    return all(int(x) <= MASK for x in a[:12])


def class_values(V, rnd, k=12):
    """boundary values of class V (integers in [0, V p]) and k random ones; 'all limbs at 2^30 - 1 up to the bound': the largest such
    value below V p, and the pattern with a zero top limb"""
    top = (V * P) >> 360
    ones = (1 << 360) - 1
    vals = [0, 1, P - 1, P, min(2 * P - 1, V * P), V * P - 1, V * P, ones, ((top - 1) << 360) | ones, (top << 360)]
    vals += [rnd.randrange(V * P + 1) for _ in range(k)]
    return [v for v in vals if 0 <= v <= V * P]


def mont(ab):
    """(ab + m p) / R' with m = -ab p^-1 mod R': the exact integer the multiplier returns"""
    m = (-ab * pow(P, -1, RP)) % RP
    assert (ab + m * P) % RP == 0
    return (ab + m * P) // RP


def mul_out(prod):
    return prod // 630 + 2
