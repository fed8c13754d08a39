"""BLS12-377 for the tests: a PRIVATE copy of the Python reference (oracle/pyref.py) that knows the curve.

oracle/pyref.py has no BLS12-377 and stays as it is (its golden files with it), but it is generic over its FIELDS / CURVES
dictionaries.  This module loads that file a second time under another module name and adds the two fields and the curve to the
copy only: the module every other test imports as `pyref` keeps its three curves (tests/test_bls12_377_cpu.py checks that).
The C++ oracle does know the curve (id 3): tests/test_oracle_bls12_377_cpu.py holds it against this copy, tests/oracle_lib.py takes
the curve's moduli from here, and the device tests of the curve check against both.  The host drivers under tests/cpp and the
workers of poly_commit_amd/sharded.py are not run for the curve.

`R` is the copy; `edge_keys` / `edge_scalars` are the MSM edge sets both the device and the oracle run; the helpers below turn its Python integers into the C ABI's buffers (little-endian 64-bit limbs, Montgomery form
where the ABI wants it) and back.  `probe()` is tests/harness/probe.py loaded the same way, with the copy as its reference, so that
its case tables and checks run for a field it does not list.
"""
import importlib.util
import os
import random

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CURVE, FQ, FR = "bls12_377", "bls12_377_fq", "bls12_377_fr"

# The constants of the curve as published (y^2 = x^3 + 1 over Fq; G1 generator of ark-bls12-377).  Multiplicative generators:
# arkworks' choice, from memory -- Fr's decides the NTT's omega.
P = 0x1ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001
RMOD = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
GX = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
GY = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
FQ_GEN, FR_GEN = 15, 22


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("_pyref_bls12_377", os.path.join(ROOT, "oracle", "pyref.py"))
R.FIELDS[FQ] = dict(p=P, gen=FQ_GEN, limbs64=6)
R.FIELDS[FR] = dict(p=RMOD, gen=FR_GEN, limbs64=4)
R.CURVES[CURVE] = dict(fq=FQ, fr=FR, b=1, gx=GX, gy=GY)
G = (GX, GY)

RQ = 1 << 384        # Montgomery radix of Fq (12 words)
RR = 1 << 256        # ... of Fr (8 words)

_probe = None


def probe():
    """tests/harness/probe.py under another module name, its reference rebound to the copy above"""
    global _probe
    if _probe is None:
        _probe = _load("_probe_bls12_377", os.path.join(ROOT, "tests", "harness", "probe.py"))
        _probe.R = R
    return _probe


# ---- integers <-> ABI buffers --------------------------------------------------------------------------------------------------------

def limbs(vals, n64):
    """integers -> (len, n64) uint64, little-endian limbs"""
    return np.frombuffer(b"".join(int(v).to_bytes(8 * n64, "little") for v in vals), dtype=np.uint64).reshape(len(vals), n64).copy()


def ints(arr):
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return [int.from_bytes(row.tobytes(), "little") for row in a.reshape(-1, a.shape[-1])]


def fr(vals):
    """canonical scalars as the ABI takes them (PC_SCALARS_CANONICAL)"""
    return limbs([v % RMOD for v in vals], 4)


def fr_mont(vals):
    return limbs([v * RR % RMOD for v in vals], 4)


def fr_from_mont(arr):
    ri = pow(RR, -1, RMOD)
    return [v * ri % RMOD for v in ints(arr)]


def point(A):
    """an affine point (or None) as x || y in Montgomery form, 12 limbs; infinity = all zero"""
    if A is None:
        return np.zeros(12, dtype=np.uint64)
    return limbs([A[0] * RQ % P, A[1] * RQ % P], 6).reshape(12)


def points(pts):
    return np.stack([point(A) for A in pts]) if len(pts) else np.zeros((0, 12), dtype=np.uint64)


def point_of(xy):
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(12)
    if not xy.any():
        return None
    ri = pow(RQ, -1, P)
    x, y = ints(xy.reshape(2, 6))
    return (x * ri % P, y * ri % P)


_bases = {}


def gen_bases(n):
    """P_i = (i + 1) G, i < n (the copy's gen_bases, kept for the session: every test that asks for fewer takes a prefix)"""
    have = _bases.get("pts", [])
    if len(have) < n:
        have = R.gen_bases(CURVE, n)
        _bases["pts"] = have
        _bases["words"] = points(have)
    return have[:n], np.ascontiguousarray(_bases["words"][:n])


def mul_g(k):
    return R.ec_mul(CURVE, k % RMOD, G)


def closed_form(scalars, first=1):
    """sum_i k_i P_i for P_i = (first + i) G: one scalar multiplication"""
    return mul_g(sum(k * (first + i) for i, k in enumerate(scalars)))


# ---- the edge sets of the MSM tests (the device tests and the C++ oracle's own tests run the same ones) -------------------------------

def edge_keys(n):
    """(name, discrete logarithms) of the keys of the edge sets; d = 0 is the (0, 0) infinity base, d < 0 a negated point"""
    plain = [i + 1 for i in range(n)]
    with_inf = list(plain)
    with_inf[7] = 0
    with_inf[min(100, n - 1)] = with_inf[min(100, n - 1) - 1]                        # a repeated base beside its copy
    same = [7] * n                                                                     # P + P in every bucket that holds two entries
    pairs = [(i // 2 + 1) * (1 if i % 2 == 0 else -1) for i in range(n)]               # P beside -P
    return {"plain": plain, "infinity and a repeated base": with_inf, "one base": same, "P beside -P": pairs}


def edge_scalars(n, seed):
    rnd = random.Random(seed)
    one = rnd.randrange(RMOD)
    pair_vals = [rnd.randrange(RMOD) for _ in range((n + 1) // 2)]
    return {
        "zeros": [0] * n, "ones": [1] * n, "r-1": [RMOD - 1] * n, "alternating 0 and r-1": [0 if i % 2 == 0 else RMOD - 1 for i in range(n)],
        "one scalar repeated": [one] * n,                                               # one bucket per window spans every chunk
        "equal in pairs": [pair_vals[i // 2] for i in range(n)],                       # with P beside -P: everything but the last cancels
        "top window only": [((i % 0x12) + 1) << 248 for i in range(n)],
        "just below r": [RMOD - 1 - (i << 200) for i in range(n)],                        # the signed digits' carry out of the top window
        "random": [rnd.randrange(RMOD) for _ in range(n)],
    }
