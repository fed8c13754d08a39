"""Case tables and checks of the sample_generators probe (tests/hip/probe_te_setup.hip): shared by tests/test_te_setup_cpu.py, which
runs them through the host build of the probe, and tests/test_te_setup_gpu.py, which runs them on the device and also compares every
output word with the host build's -- the way tests/harness/teprobe.py serves the twisted Edwards law.

The references are tests/harness/te_setup.py (from_random_bytes and sample_generators over Python integers), hashlib's blake2s and
Python integers; nothing is taken from the code under test.  Every check takes `probe` (the library under test) and `host` (the host
build; the same object in the CPU suite) and returns its lane count: the tests assert the exact number."""
import ctypes as C
import functools
import random

import numpy as np

from harness import te_setup as S
from harness import teprobe as T
from harness import teref as E

Q = E.Q
FN, XW = T.FN, T.XW
TRY_CODE = {S.ACCEPT: 0, S.RANGE: 1, S.NON_SQUARE: 2}      # pc::TE_TRY_* (csrc/te_setup.hpp)
NAMES = (b"", S.PROTOCOL_NAME, bytes(range(1, 49)))         # 0, 10 and 48 bytes: messages of 8 / 16, 18 / 26 and 56 / 64 bytes


def mont_words(vals):
    return T.probe().pack([v * T.MONT % Q for v in vals], FN)


def from_mont(rows):
    vals = T.probe().unpack(rows)
    assert all(v < Q for v in vals), "a residue left [0, q)"
    return [v * T.MONT_INV % Q for v in vals]


# ---- the square root ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def sqrt_cases():
    """0, 1, 4, q - 1, and for every k in 0..32 three values v whose v^t has order exactly 2^k: c^(2^(32 - k)) s with c = z^t for a
    non-square z and s of odd order.  k = 32 gives the non-squares."""
    s2, t = 32, (Q - 1) >> 32
    assert t % 2 == 1
    z = next(z for z in range(2, 100) if pow(z, (Q - 1) // 2, Q) == Q - 1)
    c = pow(z, t, Q)
    rnd = random.Random(3232)
    vals = [0, 1, 4, Q - 1]
    for k in range(s2 + 1):
        for _ in range(3):
            s = pow(rnd.randrange(2, Q), 1 << s2, Q)
            v = pow(c, 1 << (s2 - k), Q) * s % Q
            vt = pow(v, t, Q)
            assert pow(vt, 1 << k, Q) == 1 and (k == 0 or pow(vt, 1 << (k - 1), Q) != 1)
            vals.append(v)
    return tuple(vals)


def check_sqrt(probe_, host):
    vals = sqrt_cases()
    inp = mont_words(vals)

    def run(pr):
        out = np.zeros((len(vals), FN + 1), dtype=np.uint32)
        pr.call("pc_probe_te_setup_sqrt", C.c_size_t(len(vals)), T.p32(inp), T.p32(out))
        return out
    out = T.twin("te_setup sqrt", probe_, host, run)
    roots = from_mont(out[:, :FN])
    for i, (v, r) in enumerate(zip(vals, roots)):
        want = 1 if S.is_square(v) else 0
        assert out[i, FN] == want, "sqrt lane %d: %x is %sa square" % (i, v, "" if want else "not ")
        assert r * r % Q == (v if want else 0), "sqrt lane %d: the root of %x squares to something else" % (i, v)
    assert [int(f) for f in out[4:, FN]] == [1] * (3 * 32) + [0] * 3
    return len(vals)


# ---- the digest of a lane's message ------------------------------------------------------------------------------------------------

DIGEST_I = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1)
DIGEST_J = (0, 1, (1 << 32) + 5)


def check_digest(probe_, host):
    lanes = 0
    for name in NAMES:
        cases = [(i, None) for i in DIGEST_I] + [(i, j) for i in DIGEST_I for j in DIGEST_J]
        inp = np.array([[i & 0xffffffff, i >> 32, 0 if j is None else 1, (j or 0) & 0xffffffff, (j or 0) >> 32] for i, j in cases], dtype=np.uint32)

        def run(pr):
            out = np.zeros((len(cases), 8), dtype=np.uint32)
            pr.call("pc_probe_te_setup_digest", name, C.c_size_t(len(name)), C.c_size_t(len(cases)), T.p32(inp), T.p32(out))
            return out
        out = T.twin("te_setup digest", probe_, host, run)
        for k, (i, j) in enumerate(cases):
            assert out[k].tobytes() == S.digest(name, i, j), "digest of a %d-byte name, i = %d, j = %s" % (len(name), i, j)
        lanes += len(cases)
    assert {len(n) + 8 for n in NAMES} | {len(n) + 16 for n in NAMES} == {8, 16, 18, 26, 56, 64}
    return lanes


# ---- from_random_bytes -------------------------------------------------------------------------------------------------------------

def crafted(y, flag):
    return (y | (flag << 255)).to_bytes(32, "little")


@functools.lru_cache(None)
def y_with(square):
    return next(y for y in range(2, 1000) if S.is_square(S.x2_of_y(y)) == square and S.x2_of_y(y) != 0)


@functools.lru_cache(None)
def try_cases():
    """the crafted inputs -- y = q - 1, 1, 0, q, 2^255 - 1, a y whose x^2 is a non-square, one whose x^2 is a square, each with the flag
    clear and set -- and every digest the indices 0..15 of the reference's name consume"""
    ys = [Q - 1, 1, 0, Q, (1 << 255) - 1, y_with(False), y_with(True)]
    cases = [crafted(y, f) for y in ys for f in (0, 1)]
    for i in range(16):
        n = len(S.trace(S.PROTOCOL_NAME, i)[2])
        cases += [S.digest(S.PROTOCOL_NAME, i)] + [S.digest(S.PROTOCOL_NAME, i, j) for j in range(n - 1)]
    return tuple(cases)


def check_try(probe_, host):
    cases = try_cases()
    inp = np.frombuffer(b"".join(cases), dtype=np.uint32).reshape(len(cases), 8).copy()

    def run(pr):
        out = np.zeros((len(cases), 1 + 2 * FN), dtype=np.uint32)
        pr.call("pc_probe_te_setup_try", C.c_size_t(len(cases)), T.p32(inp), T.p32(out))
        return out
    out = T.twin("te_setup from_random_bytes", probe_, host, run)
    xs, ys = from_mont(out[:, 1:1 + FN]), from_mont(out[:, 1 + FN:])
    seen = set()
    for k, d in enumerate(cases):
        p, why = S.try_bytes(d)
        seen.add(why)
        assert out[k, 0] == TRY_CODE[why], "from_random_bytes lane %d: outcome %d, want %s" % (k, out[k, 0], why)
        assert (xs[k], ys[k]) == (p if p is not None else (0, 0)), "from_random_bytes lane %d: another point" % k
    assert seen == set(TRY_CODE)
    return len(cases)


# ---- the whole per-index body ------------------------------------------------------------------------------------------------------

SAMPLE_RANGES = ((0, 64), (1008, 1), ((1 << 32) - 1, 2))      # indices 0..63, the 16-digest index, the two sides of le64's word edge


def run_sample(pr, name, first, n):
    ext, dg, failed = np.zeros((n, XW), dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    pr.call("pc_probe_te_setup_sample", name, C.c_size_t(len(name)), C.c_uint64(first), C.c_size_t(n), T.p32(ext), T.p32(dg), T.p32(failed))
    return np.concatenate([ext.reshape(-1), dg, failed])


def check_sample(probe_, host):
    lanes = 0
    for first, n in SAMPLE_RANGES:
        out = T.twin("te_setup sample", probe_, host, lambda pr: run_sample(pr, S.PROTOCOL_NAME, first, n))
        ext, dg, failed = out[:n * XW].reshape(n, XW), out[n * XW:n * XW + n], out[-1]
        pts, counts = S.generators(S.PROTOCOL_NAME, first, n)
        assert failed == 0 and [int(x) for x in dg] == counts, "digest counts from index %d: %s, want %s" % (first, list(dg), counts)
        for k in range(n):
            T.check_ext("generator %d" % (first + k), ext[k], pts[k])
        lanes += n
    return lanes
