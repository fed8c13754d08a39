#!/usr/bin/env python3
"""Generate poly_commit_amd/csrc/te_constants.h: the constants of the twisted Edwards curve ed_on_bls12_381 (JubJub),

    a x^2 + y^2 = 1 + d x^2 y^2   over Fq = BLS12-381's Fr,   a = -1,  d = -10240/10241,

in the struct shapes of field_constants.h (32-bit limbs, Montgomery form): the scalar field pc_ed_on_bls12_381_fr and the curve
struct pc_te_ed_on_bls12_381 (FqP = pc_bls12_381_fr of field_constants.h, FrP, D, D2 = 2 d, GX, GY -- arkworks' generator).
Every fact the device code relies on is asserted here before anything is written: a is a square and d is not (the a = -1 extended
formulas are then complete), r is prime, the cofactor is 8, the generator is on the curve and r G = (0, 1).

  python tools/gen_te_constants.py            writes the header
  python tools/gen_te_constants.py --stdout   prints it (tests/test_te_cpu.py compares this with the committed file)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "poly_commit_amd", "csrc", "te_constants.h")

Q = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001      # BLS12-381 Fr
R = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7      # the prime subgroup order
COFACTOR = 8
A = Q - 1
D = (-10240 * pow(10241, -1, Q)) % Q
GX = 8076246640662884909881801758704306714034609987455869804520522091855516602923
GY = 13262374693698910701929044844600465831413122818447359594527400194675274060458
SQRT_S = 32                                  # the 2-adicity of q - 1
SQRT_T = (Q - 1) >> SQRT_S
SQRT_Z = 5                                   # the least non-square of Fq
SQRT_C = pow(SQRT_Z, SQRT_T, Q)


def on_curve(p):
    x, y = p
    return (A * x * x + y * y - 1 - D * x * x % Q * y * y) % Q == 0


def add(p, q):
    """the complete affine law (no exceptional inputs for a square a and a non-square d)"""
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 % Q * y1 * y2 % Q
    x3 = (x1 * y2 + y1 * x2) * pow(1 + t, -1, Q) % Q
    y3 = (y1 * y2 - A * x1 * x2) * pow(1 - t, -1, Q) % Q
    return (x3, y3)


def mul(k, p):
    acc = (0, 1)
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, p)
    return acc


def is_prime(n):
    """Miller-Rabin over the first 24 prime bases"""
    if n < 2:
        return False
    small = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89]
    for s in small:
        if n % s == 0:
            return n == s
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def check_facts():
    assert D == 0x2a9318e74bfa2b48f5fd9207e6bd7fd4292d7f6d37579d2601065fd6d6343eb1
    assert pow(A, (Q - 1) // 2, Q) == 1, "a = -1 must be a square in Fq"
    assert pow(D, (Q - 1) // 2, Q) == Q - 1, "d must be a non-square in Fq"
    assert is_prime(Q) and is_prime(R) and R.bit_length() == 252
    assert ((R - 1) & -(R - 1)) == 2, "the 2-adicity of r - 1 is 1: no NTT over this field"
    # Hasse: the group order 8 r lies within 2 sqrt(q) of q + 1
    assert (COFACTOR * R - Q - 1) ** 2 <= 4 * Q
    G = (GX, GY)
    assert on_curve(G) and mul(R, G) == (0, 1) and G != (0, 1)
    # the low-order points: (0, -1) of order 2, y = 0 of order 4, R * (a point with y = 11) of order 8
    assert on_curve((0, Q - 1)) and add((0, Q - 1), (0, Q - 1)) == (0, 1)
    x4 = sqrt_mod(pow(A, -1, Q))      # y = 0: a x^2 = 1
    assert on_curve((x4, 0)) and mul(2, (x4, 0)) == (0, Q - 1)
    y = 11
    x2 = (1 - y * y) * pow(A - D * y * y, -1, Q) % Q
    t8 = mul(R, (sqrt_mod(x2), y))
    assert on_curve(t8) and mul(4, t8) == (0, Q - 1) and mul(8, t8) == (0, 1)
    # the square root in Fq (csrc/te_setup.hpp): q - 1 = 2^32 t with t odd, c = z^t of order exactly 2^32 for the non-square z,
    # and a / d a non-square, so that the denominator a - d y^2 of the decompression is never zero
    assert SQRT_T % 2 == 1 and Q - 1 == SQRT_T << SQRT_S
    assert pow(SQRT_Z, (Q - 1) // 2, Q) == Q - 1
    assert pow(SQRT_C, 1 << (SQRT_S - 1), Q) == Q - 1 and pow(SQRT_C, 1 << SQRT_S, Q) == 1
    assert ((SQRT_T - 1) // 2).bit_length() <= 32 * 7
    assert pow(A * pow(D, -1, Q) % Q, (Q - 1) // 2, Q) == Q - 1


def sqrt_mod(v):
    """Tonelli-Shanks in Fq (asserts that v is a square)"""
    v %= Q
    assert pow(v, (Q - 1) // 2, Q) == 1
    s, t = 0, Q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (Q - 1) // 2, Q) != Q - 1:
        z += 1
    m, c, tt, r = s, pow(z, t, Q), pow(v, t, Q), pow(v, (t + 1) // 2, Q)
    while tt != 1:
        i, x = 0, tt
        while x != 1:
            x, i = x * x % Q, i + 1
        b = pow(c, 1 << (m - i - 1), Q)
        m, c = i, b * b % Q
        tt, r = tt * c % Q, r * b % Q
    assert r * r % Q == v
    return r


def fmt(v, n=8):
    return "{" + ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(n)) + "}"


def render():
    check_facts()
    n = 8
    o = ["// GENERATED by tools/gen_te_constants.py -- do not edit.", "#pragma once", "#include <stdint.h>", '#include "field_constants.h"', ""]
    rm = (1 << (32 * n)) % R
    o += ["// the scalar field of ed_on_bls12_381 (JubJub): r - 1 = 2 * odd, so the only two-adic root is -1 and there is no NTT over it",
          "struct pc_ed_on_bls12_381_fr {",
          f"  static constexpr int N = {n};",
          f"  static constexpr int BITS = {R.bit_length()};",
          "  static constexpr int TWO_ADICITY = 1;",
          f"  static constexpr uint32_t INV = 0x{(-pow(R, -1, 1 << 32)) % (1 << 32):08x}u;",
          f"  static constexpr uint32_t MOD[{n}] = {fmt(R)};",
          f"  static constexpr uint32_t ONE[{n}] = {fmt(rm)};   // R mod p",
          f"  static constexpr uint32_t R2[{n}] = {fmt(rm * rm % R)};    // R^2 mod p",
          "  // -1 in Montgomery form",
          f"  static constexpr uint32_t ROOT[{n}] = {fmt((R - 1) * rm % R)};",
          '  static constexpr const char* NAME = "ed_on_bls12_381_fr";',
          "};", ""]
    qm = (1 << (32 * n)) % Q
    o += ["// a x^2 + y^2 = 1 + d x^2 y^2 over BLS12-381's Fr with a = -1 (a square) and d = -10240/10241 (a non-square): the a = -1",
          "// extended-coordinate formulas are complete.  Cofactor 8; GX, GY: arkworks' generator of the prime-order subgroup.",
          "struct pc_te_ed_on_bls12_381 {",
          "  typedef pc_bls12_381_fr FqP;",
          "  typedef pc_ed_on_bls12_381_fr FrP;",
          f"  static constexpr int COFACTOR = {COFACTOR};",
          f"  static constexpr uint32_t D[{n}] = {fmt(D * qm % Q)};    // Montgomery",
          f"  static constexpr uint32_t D2[{n}] = {fmt(2 * D * qm % Q)};   // 2 d, Montgomery",
          f"  static constexpr uint32_t GX[{n}] = {fmt(GX * qm % Q)};  // generator, Montgomery",
          f"  static constexpr uint32_t GY[{n}] = {fmt(GY * qm % Q)};",
          "  // the square root in Fq (te_setup.hpp): q - 1 = 2^SQRT_S * t, SQRT_EXP = (t - 1) / 2, SQRT_C = z^t of order 2^SQRT_S (z = 5), Montgomery",
          f"  static constexpr int SQRT_S = {SQRT_S};",
          "  static constexpr int SQRT_EXP_WORDS = 7;",
          f"  static constexpr uint32_t SQRT_EXP[7] = {fmt((SQRT_T - 1) // 2, 7)};",
          f"  static constexpr uint32_t SQRT_C[{n}] = {fmt(SQRT_C * qm % Q)};",
          '  static constexpr const char* NAME = "ed_on_bls12_381";',
          "};", ""]
    return "\n".join(o)


if __name__ == "__main__":
    text = render()
    if "--stdout" in sys.argv:
        sys.stdout.write(text)
    else:
        with open(OUT, "w") as fh:
            fh.write(text)
        print("wrote", OUT)
