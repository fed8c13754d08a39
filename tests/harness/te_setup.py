"""Pure-Python restatement of InnerProductArgPC::setup / trim over ed_on_bls12_381 (ipa_pc/mod.rs:302-325, 344-400) for the tests of the
device path (csrc/te_setup.hpp, abi_te_setup.hip, te_ipa.setup / trim): `sample_generators` with D = Blake2s256 and
twisted_edwards::Affine::from_random_bytes, over harness/teref.py on Python integers.

from_random_bytes is restated from the published behaviour of ark-ec / ark-ff 0.5 and, like the transcript conventions of
harness/te_ipa.py, NOT confirmed against the crates:
  the 32 bytes are a little-endian integer v; TEFlags has one flag bit, 255 + 1 = 256 bits, so the flag is bit 255 (bit 7 of byte 31)
  y = v mod 2^255, None at y >= q;  x^2 = (1 - y^2) / (a - d y^2), None where that is a non-square (0 is a square with root 0)
  of the two roots the larger canonical integer is taken when the flag is set, the smaller when it is clear
Nothing here is taken from the code under test."""
import functools
import hashlib

from . import teref as E

Q = E.Q
PROTOCOL_NAME = b"PC-DL-2020"
ACCEPT, RANGE, NON_SQUARE = "accept", "y >= q", "non-square"


def is_square(v):
    v %= Q
    return v == 0 or pow(v, (Q - 1) // 2, Q) == 1


def sqrt(v):
    """either root of a square; 0 for 0"""
    v %= Q
    return 0 if v == 0 else E._sqrt(v)


def x2_of_y(y):
    return (1 - y * y) * pow(E.A - E.D * y * y, -1, Q) % Q      # a / d is a non-square: the denominator is never 0


def try_bytes(digest):
    """Affine::from_random_bytes on 32 bytes -> (point or None, reason)"""
    v = int.from_bytes(digest[:32], "little")
    flag, y = v >> 255, v & ((1 << 255) - 1)
    if y >= Q:
        return None, RANGE
    x2 = x2_of_y(y)
    if not is_square(x2):
        return None, NON_SQUARE
    x = sqrt(x2)
    nx = (Q - x) % Q
    lo, hi = min(x, nx), max(x, nx)
    return ((hi if flag else lo), y), ACCEPT


def digest(name, i, j=None):
    return hashlib.blake2s(name + i.to_bytes(8, "little") + (b"" if j is None else j.to_bytes(8, "little"))).digest()


def trace(name, i):
    """-> (the point before the cofactor multiplication, the accepted digest, the outcome of every digest in order)"""
    h = digest(name, i)
    g, why = try_bytes(h)
    reasons, j = [why], 0
    while g is None:
        h = digest(name, i, j)
        g, why = try_bytes(h)
        reasons.append(why)
        j += 1
    return g, h, reasons


@functools.lru_cache(None)
def generator(name, i):
    """generator i of sample_generators: (8 * g, the number of digests consumed); computed once per (name, i) and shared"""
    g, _, reasons = trace(name, i)
    return E.mul(E.COFACTOR, g), len(reasons)


def generators(name, first, count):
    """-> (points, digest counts) of the indices [first, first + count)"""
    out = [generator(name, first + k) for k in range(count)]
    return [p for p, _ in out], [c for _, c in out]


def pow2_at_least(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def setup(max_degree, name=PROTOCOL_NAME):
    """InnerProductArgPC::setup: max_degree + 1 rounded up to a power of two; the reference pops h first, so h is the last generator"""
    n = pow2_at_least(max_degree + 1)
    max_degree = n - 1
    gens, _ = generators(name, 0, max_degree + 3)
    return dict(comm_key=gens[:max_degree + 1], s=gens[max_degree + 1], h=gens[max_degree + 2], max_degree=max_degree)


def trim(pp, supported_degree):
    n = pow2_at_least(supported_degree + 1)
    supported_degree = n - 1
    if supported_degree > pp["max_degree"]:
        raise ValueError("TrimmingDegreeTooLarge")
    return dict(comm_key=pp["comm_key"][:supported_degree + 1], s=pp["s"], h=pp["h"], supported_degree=supported_degree, max_degree=pp["max_degree"])
