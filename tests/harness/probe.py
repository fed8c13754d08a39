"""Case tables and checks of the primitive probe (tests/hip): shared by tests/test_device_primitives_cpu.py, which runs them through
the host build of the probe bodies, and tests/test_device_primitives_gpu.py, which runs them on the device and also compares every
output word with the host build's.

Operand sets are built here from the moduli (oracle/pyref.py), not taken from the code under test; expected values are exact Python
integers.  Every check takes `probe` (the library under test) and `host` (the host build: it prepares chained operands and is the
word-for-word twin; the same object in the CPU suite).
"""
import ctypes as C
import importlib.util
import itertools
import os
import random
import subprocess
import tempfile

import numpy as np

import pyref as R
from harness import fq30ref as Q
from harness import g2ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIP_DIR = os.path.join(ROOT, "tests", "hip")
UNSUPPORTED = -1

FIELDS = ["bls12_381_fq", "bls12_381_fr", "bn254_fq", "bn254_fr", "pallas_fq", "pallas_fr"]
G1_CURVES = ["bls12_381", "bn254", "pallas"]
GROUPS = G1_CURVES + ["bls12_381_g2"]

# probe::FieldOp, probe::Fq30Op, probe::Fq2Op, probe::CurveOp (tests/hip/probe_bodies.hpp)
(F_MUL, F_SQR, F_MUL_ADD_MUL, F_FROM_MONT, F_TO_MONT, F_ADD, F_SUB, F_DBL, F_NEG, F_INV, F_MUL_LZ, F_SQR_LZ, F_MUL_ADD_MUL_LZ, F_SUB_LZ,
 F_DBL_LZ, F_NEG_LZ, F_NEG_LZ_CANONICAL, F_IS_ZERO_LZ, F_CANON1, F_CANON) = range(20)
(Q_MUL_64_2, Q_MUL_66_8, Q_MUL_64_8, Q_MUL_2_8, Q_MUL_2_2, Q_REDUCE, Q_SQR_66, Q_MUL_ADD_MUL, Q_SUB_64, Q_SUB_2, Q_SUB_14, Q_SUB_DBL_4,
 Q_NEG_64, Q_FROM32, Q_TO32, Q_IS_ZERO_MODP_66, Q_IS_ZERO_EXACT, Q_ONE) = range(18)
E_MUL, E_SQR, E_MUL_ADD_MUL, E_INV, E_ADD, E_SUB, E_NEG = range(7)
C_ADD_AFFINE, C_ADD_AFFINE_LZ, C_ADD, C_DBL, C_DBL_AFFINE, C_TO_AFFINE = range(6)


# ---- the two builds of the probe ---------------------------------------------------------------------------------------------------

def _build_module():
    spec = importlib.util.spec_from_file_location("_pc_build", os.path.join(ROOT, "poly_commit_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Probe:
    failed = None

    def __init__(self, path, name):
        self.lib, self.name = C.CDLL(path), name

    def raw(self, entry, *args):
        fn = getattr(self.lib, entry)
        fn.restype = C.c_int
        return fn(*args)

    def call(self, entry, *args):
        # a HIP error is not retried, and nothing more is launched by this process after one
        assert Probe.failed is None, "not run: an earlier probe call failed (%s)" % Probe.failed
        st = self.raw(entry, *args)
        if st != 0:
            Probe.failed = "%s (%s build of the probe) returned HIP status %d" % (entry, self.name, st)
        assert st == 0, Probe.failed


_probes = {}


def host_probe():
    """tests/hip/libpc_probe_host.so: the probe units compiled by g++, the bodies looped over on the host; built on demand"""
    if "host" not in _probes:
        b = _build_module()
        so = os.path.join(HIP_DIR, "libpc_probe_host.so")
        csrc = os.path.join(ROOT, "poly_commit_amd", "csrc")
        srcs = b.probe_sources() + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".h"))]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            with tempfile.TemporaryDirectory() as tmp:
                objs = []
                for src, k in b.PROBE_UNITS:
                    objs.append(os.path.join(tmp, os.path.basename(b.probe_object((src, k)))))
                    subprocess.check_call(["g++", "-x", "c++", "-O2", "-std=c++17", "-fPIC", *([] if k is None else ["-DPROBE_SET=%d" % k]),
                                           "-c", os.path.join(HIP_DIR, src), "-o", objs[-1]])
                out = "%s.%d.tmp" % (so, os.getpid())                  # (xdist workers may build at once: each its own file, renamed into place)
                subprocess.check_call(["g++", "-shared", "-fPIC", "-o", out, *objs])
                os.replace(out, so)
        _probes["host"] = Probe(so, "host")
    return _probes["host"]


def device_probe():
    """tests/hip/libpc_probe.so, built for gfx950 by poly_commit_amd/build.py (PC_PROBE_LIB: another build of it); never built here"""
    if "device" not in _probes:
        so = os.environ.get("PC_PROBE_LIB") or os.path.join(HIP_DIR, "libpc_probe.so")
        assert os.path.exists(so), "%s is missing: run build() (python __graft_entry__.py) first" % so
        _probes["device"] = Probe(so, "device")
    return _probes["device"]


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


# ---- words <-> integers ------------------------------------------------------------------------------------------------------------

def pack(vals, n):
    """integers -> len(vals) x n little-endian 32-bit words"""
    return np.frombuffer(b"".join(v.to_bytes(4 * n, "little") for v in vals), dtype=np.uint32).reshape(len(vals), n).copy()


def unpack(arr):
    return [int.from_bytes(np.ascontiguousarray(row).tobytes(), "little") for row in arr]


def pack13(vals):
    return np.array([Q.to13(v) for v in vals], dtype=np.uint32).reshape(len(vals), 13)


def dedupe(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---- operand sets ------------------------------------------------------------------------------------------------------------------

class Field:
    def __init__(self, name):
        self.name = name
        self.p = R.FIELDS[name]["p"]
        self.N = 2 * R.FIELDS[name]["limbs64"]
        self.R = 1 << (32 * self.N)
        self.Ri = pow(self.R, -1, self.p)
        self.pinv = pow(self.p, -1, self.R)
        bits = self.p.bit_length()
        self.lazy = bits + 2 <= 32 * self.N               # fp32.hpp LAZY_OK: 4p fits the limbs
        self.lazy_fused = bits + 3 <= 32 * self.N         # LAZY_FUSED_OK: R >= 8p
        curve, which = name.rsplit("_", 1)
        self.entry, self.which = "pc_probe_field_" + curve, 0 if which == "fq" else 1

    def limbs(self, limb):
        return sum(x << (32 * i) for i, x in enumerate(limb))

    def canonical_set(self, seed=1):
        p, N = self.p, self.N
        vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, self.R % p, self.R * self.R % p]
        for j in range(N):
            vals += [v for v in (1 << (32 * j), (1 << (32 * j)) - 1) if v < p]
        vals.append((((p >> (32 * (N - 1))) - 1) << (32 * (N - 1))) | ((1 << (32 * (N - 1))) - 1))
        # bit 31 of every limb set / clear, alternating all-ones and zero limbs: the doubled limbs d = a << 1 of the squaring carry a
        # bit out of every limb, so the adjacent cross term needs dm (the limb shifted WITHOUT its neighbour's bit)
        pats = [[0x80000000] * N, [0x7fffffff] * N, [0xffffffff, 0] * (N // 2), [0, 0xffffffff] * (N // 2)]
        vals += [v if v < p else v % p for v in (self.limbs(x) for x in pats)]
        rnd = random.Random(seed)
        vals += [rnd.randrange(p) for _ in range(32)]
        assert all(0 <= v < p for v in vals)
        return dedupe(vals)

    def lazy_set(self, seed=1):
        p, c = self.p, self.canonical_set(seed)
        return dedupe(c + [p, p + 1, 2 * p - 1, 2 * p] + [x + p for x in c])

    def mont_exact(self, s):
        """(s + m p) / R with m = -s p^-1 mod R: the integer a Montgomery reduction of s returns before any subtraction"""
        m = (-s * self.pinv) % self.R
        return (s + m * self.p) // self.R


def extremes(vals, k=6):
    """indices of the k smallest and k largest members"""
    order = sorted(range(len(vals)), key=lambda i: vals[i])
    return dedupe(order[:k] + order[-k:])


def tuples4(sets, worst, seed, nrand=400):
    """four-operand cases as index tuples: the worst tuple, the cross product of the six smallest and six largest members per argument,
    and `nrand` seeded random tuples"""
    rnd = random.Random(seed)
    idx = [tuple(s.index(w) for s, w in zip(sets, worst))]
    idx += list(itertools.product(*(extremes(s) for s in sets)))
    idx += [tuple(rnd.randrange(len(s)) for s in sets) for _ in range(nrand)]
    return idx


def run_op(probe, entry, pre, width, cols, out_width=None):
    """one launch: cols = up to four (n x width) operand arrays; returns the (n x out_width) result words"""
    n = len(cols[0])
    inp = np.zeros((n, 4 * width), dtype=np.uint32)
    for k, c in enumerate(cols):
        inp[:, k * width:(k + 1) * width] = c
    out = np.zeros((n, out_width or width), dtype=np.uint32)
    probe.call(entry, *pre, C.c_size_t(n), p32(inp), p32(out))
    return out


def expect(name, got, want, operands):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            raise AssertionError("%s: lane %d, operands %s: got %s, want %s" % (name, i, [hex(x) if isinstance(x, int) else x for x in operands(i)],
                                                                                 hex(g) if isinstance(g, int) else g, hex(w) if isinstance(w, int) else w))
    assert len(got) == len(want)


def same_words(name, a, b, operands=None):
    if not np.array_equal(a, b):
        i = int(np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0][0])
        raise AssertionError("%s: device and host words differ at lane %d%s: %s vs %s" % (
            name, i, "" if operands is None else ", operands %s" % [hex(x) if isinstance(x, int) else x for x in operands(i)], a[i], b[i]))


# ---- Fd<P> -------------------------------------------------------------------------------------------------------------------------

FIELD_GROUPS = ["products", "fused", "additive", "inv", "lazy_products", "lazy_fused", "lazy_additive"]


def field_cases(f, group):
    """-> list of (name, op, operand value lists per argument, index tuples, expected(values) -> int, bound or None)"""
    p, Ri, Rm = f.p, f.Ri, f.R
    Cn, Lz = f.canonical_set(), f.lazy_set()
    Lz_open = [v for v in Lz if v < 2 * p]
    cross = lambda A, B: list(itertools.product(range(len(A)), range(len(B))))
    unary = lambda A: [(i,) for i in range(len(A))]
    if group == "products":
        return [("mul", F_MUL, [Cn, Cn], cross(Cn, Cn), lambda a, b: a * b * Ri % p, p),
                ("sqr", F_SQR, [Cn], unary(Cn), lambda a: a * a * Ri % p, p),
                ("from_mont", F_FROM_MONT, [Cn], unary(Cn), lambda a: a * Ri % p, p),
                ("to_mont", F_TO_MONT, [Cn], unary(Cn), lambda a: a * Rm % p, p)]
    if group == "fused":
        return [("mul_add_mul", F_MUL_ADD_MUL, [Cn] * 4, tuples4([Cn] * 4, [p - 1] * 4, 41), lambda a, b, c, d: (a * b + c * d) * Ri % p, p)]
    if group == "additive":
        return [("add", F_ADD, [Cn, Cn], cross(Cn, Cn), lambda a, b: (a + b) % p, p),
                ("sub", F_SUB, [Cn, Cn], cross(Cn, Cn), lambda a, b: (a - b) % p, p),
                ("dbl", F_DBL, [Cn], unary(Cn), lambda a: 2 * a % p, p),
                ("neg", F_NEG, [Cn], unary(Cn), lambda a: -a % p, p)]
    if group == "inv":
        return [("inv", F_INV, [Cn], unary(Cn), lambda a: pow(a, -1, p) * Rm * Rm % p if a else 0, p)]
    assert f.lazy
    if group == "lazy_products":           # raw outputs: exactly (a b + m p) / R, below 2p
        return [("mul_lz", F_MUL_LZ, [Lz, Lz], cross(Lz, Lz), lambda a, b: f.mont_exact(a * b), 2 * p),
                ("sqr_lz", F_SQR_LZ, [Lz], unary(Lz), lambda a: f.mont_exact(a * a), 2 * p)]
    if group == "lazy_fused":              # R >= 8p: no subtraction; else ONE conditional subtraction of p (fp32.hpp, lazy reduction)
        def fused(a, b, c, d):
            v = f.mont_exact(a * b + c * d)
            return v if f.lazy_fused or v < p else v - p
        return [("mul_add_mul_lz", F_MUL_ADD_MUL_LZ, [Lz] * 4, tuples4([Lz] * 4, [2 * p] * 4, 42), fused, 2 * p)]
    if group == "lazy_additive":
        return [("sub_lz", F_SUB_LZ, [Lz, Lz], cross(Lz, Lz), lambda a, b: a - b if a >= b else a - b + 2 * p, 2 * p + 1),
                ("dbl_lz", F_DBL_LZ, [Lz_open], unary(Lz_open), lambda a: 2 * a if 2 * a < 2 * p else 2 * a - 2 * p, 2 * p),
                ("neg_lz", F_NEG_LZ, [Lz], unary(Lz), lambda a: 2 * p - a, 2 * p + 1),
                ("neg_lz_canonical", F_NEG_LZ_CANONICAL, [Cn], unary(Cn), lambda a: p - a, p + 1),
                ("is_zero_lz", F_IS_ZERO_LZ, [Lz], unary(Lz), lambda a: 1 if a % p == 0 else 0, 2),
                ("canon1", F_CANON1, [Lz_open], unary(Lz_open), lambda a: a - p if a >= p else a, p),
                ("canon", F_CANON, [Lz], unary(Lz), lambda a: a % p, p)]
    raise KeyError(group)


def check_field(probe, host, fname, group):
    f = Field(fname)
    flags = probe.raw(f.entry.replace("pc_probe_field", "pc_probe_field_lazy"), C.c_int(f.which))
    assert flags == (1 if f.lazy else 0) | (2 if f.lazy_fused else 0), "LAZY_OK / LAZY_FUSED_OK differ from the moduli's"
    if group.startswith("lazy") and not f.lazy:
        dummy = np.zeros(4 * f.N, dtype=np.uint32)
        for op in range(F_MUL_LZ, F_CANON + 1):
            assert probe.raw(f.entry, C.c_int(f.which), C.c_int(op), C.c_size_t(1), p32(dummy), p32(dummy.copy())) == UNSUPPORTED
        return 0
    lanes = 0
    for name, op, sets, idx, want_fn, bound in field_cases(f, group):
        packed = [pack(s, f.N) for s in sets]
        ia = np.array(idx, dtype=np.int64)
        cols = [packed[k][ia[:, k]] for k in range(len(sets))]
        operands = lambda i: [sets[k][idx[i][k]] for k in range(len(sets))]
        out = run_op(probe, f.entry, (C.c_int(f.which), C.c_int(op)), f.N, cols)
        got = unpack(out)
        expect("%s %s" % (fname, name), got, [want_fn(*operands(i)) for i in range(len(idx))], operands)
        assert all(g < bound for g in got), "%s %s: an output outside its documented range" % (fname, name)
        if host is not probe:
            same_words("%s %s" % (fname, name), out, run_op(host, f.entry, (C.c_int(f.which), C.c_int(op)), f.N, cols), operands)
        lanes += len(idx)
    return lanes


# ---- Fq30 --------------------------------------------------------------------------------------------------------------------------

FQ30_GROUPS = ["products", "fused", "additive", "conversions", "is_zero"]
_PINV30 = pow(Q.P, -1, Q.RP)


def _mont30(s):
    return (s + (-s * _PINV30) % Q.RP * Q.P) // Q.RP


def fq30_cases(group):
    """-> list of (name, op, operand value lists, index tuples, expected(values) -> int, class of the output or None)"""
    P = Q.P
    cross = lambda A, B: list(itertools.product(range(len(A)), range(len(B))))
    unary = lambda A: [(i,) for i in range(len(A))]
    cv = lambda V, seed, k=12: dedupe(Q.class_values(V, random.Random(seed), k))
    if group == "products":
        out = []
        for name, op, VA, VB in (("mul<64,2>", Q_MUL_64_2, 64, 2), ("mul<66,8>", Q_MUL_66_8, 66, 8), ("mul<64,8>", Q_MUL_64_8, 64, 8),
                                 ("mul<2,8>", Q_MUL_2_8, 2, 8), ("mul<2,2>", Q_MUL_2_2, 2, 2)):
            A, B = cv(VA, 300 + op), cv(VB, 400 + op)
            out.append((name, op, [A, B], cross(A, B), lambda a, b: _mont30(a * b), Q.mul_out(VA * VB)))
        A = cv(66, 306, 60)
        out.append(("sqr<66>", Q_SQR_66, [A], unary(A), lambda a: _mont30(a * a), Q.mul_out(66 * 66)))
        A = cv(64, 305, 60)
        out.append(("reduce", Q_REDUCE, [A], unary(A), lambda a: _mont30(a * (Q.RP % P)), 2))
        return out
    if group == "fused":
        V = (66, 16, 64, 2)
        sets = [cv(v, 500 + i) for i, v in enumerate(V)]
        return [("mul_add_mul<66,16,64,2>", Q_MUL_ADD_MUL, sets, tuples4(sets, [v * P for v in V], 43),
                 lambda a, b, c, d: _mont30(a * b + c * d), Q.mul_out(66 * 16 + 64 * 2))]
    if group == "additive":                # sub<V>(a, b) = a - b + V p for b <= V p; sub_dbl<V>: a - 2b + V p for 2b <= V p; classes as in add_affine
        out = []
        for name, op, VA, V, fac in (("sub<64>", Q_SUB_64, 2, 64, 1), ("sub<2>", Q_SUB_2, 8, 2, 1), ("sub<14>", Q_SUB_14, 2, 14, 1),
                                     ("sub_dbl<4>", Q_SUB_DBL_4, 10, 4, 2)):
            A, B = cv(VA, 600 + op), cv(V // fac, 700 + op)
            out.append((name, op, [A, B], cross(A, B), (lambda V, fac: lambda a, b: a - fac * b + V * P)(V, fac), VA + V))
        A = cv(64, 612, 60)
        out.append(("neg<64>", Q_NEG_64, [A], unary(A), lambda a: 64 * P - a, 64))
        return out
    raise KeyError(group)


def check_fq30(probe, host, group):
    P = Q.P
    lanes = 0
    if group in ("products", "fused", "additive"):
        for name, op, sets, idx, want_fn, cls in fq30_cases(group):
            packed = [pack13(s) for s in sets]
            ia = np.array(idx, dtype=np.int64)
            cols = [packed[k][ia[:, k]] for k in range(len(sets))]
            operands = lambda i: [sets[k][idx[i][k]] for k in range(len(sets))]
            out = run_op(probe, "pc_probe_fq30", (C.c_int(op),), 13, cols)
            assert (out[:, :12] <= Q.MASK).all(), "%s: a limb is not normalised" % name
            got = [Q.from13(r) for r in out]
            expect(name, got, [want_fn(*operands(i)) for i in range(len(idx))], operands)
            assert all(g <= cls * P for g in got), "%s: an output above its class %d" % (name, cls)
            if host is not probe:
                same_words(name, out, run_op(host, "pc_probe_fq30", (C.c_int(op),), 13, cols), operands)
            lanes += len(idx)
        return lanes

    def run(op, vals, packer=pack13, width=13):
        cols = [np.pad(packer(vals), ((0, 0), (0, 13 - width)))]
        out = run_op(probe, "pc_probe_fq30", (C.c_int(op),), 13, cols)
        if host is not probe:
            same_words("fq30 op %d" % op, out, run_op(host, "pc_probe_fq30", (C.c_int(op),), 13, cols), lambda i: [vals[i]])
        return out
    rnd = random.Random(35)
    if group == "conversions":
        # from32: a 12-word residue w <= p becomes 64 w; to32: the exact division by 64 modulo p, below 2p
        ws = dedupe(Field("bls12_381_fq").canonical_set() + [P] + [rnd.randrange(P) for _ in range(200)])
        a = run(Q_FROM32, ws, lambda v: pack(v, 12), 12)
        assert (a[:, :12] <= Q.MASK).all()
        expect("from32", [Q.from13(r) for r in a], [64 * w for w in ws], lambda i: [ws[i]])
        vs = dedupe([64 * w for w in ws] + Q.class_values(64, rnd, 100))
        back = run(Q_TO32, vs)
        assert not back[:, 12].any()
        got = unpack(back[:, :12])
        k64 = pow(64, -1, P)
        for v, g in zip(vs, got):
            k = (-v * pow(P, -1, 64)) % 64
            assert g == (v + k * P) // 64 and g < 2 * P and g % P == v * k64 % P, hex(v)
        one = run(Q_ONE, [0])
        assert Q.from13(one[0]) == Q.RP % P
        return len(ws) + len(vs) + 1
    if group == "is_zero":
        vals = []
        for k in range(67):
            vals.append(k * P)
            if k:
                vals.append(k * P - 1)
            if k < 66:
                vals += [k * P + 1, k * P + (1 << 30) * rnd.randrange(1, 1 << 200)]      # limb 0 of k p, another value
        vals += [rnd.randrange(66 * P) for _ in range(300)]
        vals = [v for v in dedupe(vals) if v <= 66 * P]
        z = run(Q_IS_ZERO_MODP_66, vals)
        expect("is_zero_modp<66>", [int(x) for x in z[:, 0]], [1 if v % P == 0 else 0 for v in vals], lambda i: [vals[i]])
        ev = [0, 1, P, 1 << 360, 1 << 30, Q.MASK, 64 * P]
        z = run(Q_IS_ZERO_EXACT, ev)
        expect("is_zero_exact", [int(x) for x in z[:, 0]], [1 if v == 0 else 0 for v in ev], lambda i: [ev[i]])
        return len(vals) + len(ev)
    raise KeyError(group)


# ---- Fq2 ---------------------------------------------------------------------------------------------------------------------------

FQ2_GROUPS = ["products", "fused", "additive", "inv"]


def fq2_set(seed=2):
    f = Field("bls12_381_fq")
    p = f.p
    b = [0, 1, p - 1, (p - 1) // 2, f.R % p, (((p >> 352) - 1) << 352) | ((1 << 352) - 1), f.limbs([0xffffffff, 0] * 6) % p]
    rnd = random.Random(seed)
    return dedupe(list(itertools.product(b, b)) + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(15)])


def pack_fq2(vals):
    return np.concatenate([pack([v[0] for v in vals], 12), pack([v[1] for v in vals], 12)], axis=1)


def check_fq2(probe, host, group):
    f = Field("bls12_381_fq")
    p, Ri, R2 = f.p, f.Ri, f.R * f.R % f.p
    S = fq2_set()
    sc = lambda v, k: (v[0] * k % p, v[1] * k % p)
    cross = list(itertools.product(range(len(S)), repeat=2))
    unary = [(i,) for i in range(len(S))]
    if group == "products":
        cases = [("mul", E_MUL, 2, cross, lambda a, b: sc(G.f2_mul(a, b), Ri)), ("sqr", E_SQR, 1, unary, lambda a: sc(G.f2_sqr(a), Ri))]
    elif group == "fused":
        idx = tuples4([S] * 4, [(p - 1, p - 1)] * 4, 44)
        cases = [("mul_add_mul", E_MUL_ADD_MUL, 4, idx, lambda a, b, c, d: sc(G.f2_mul_add_mul(a, b, c, d), Ri))]
    elif group == "additive":
        cases = [("add", E_ADD, 2, cross, G.f2_add), ("sub", E_SUB, 2, cross, G.f2_sub), ("neg", E_NEG, 1, unary, G.f2_neg)]
    else:
        cases = [("inv", E_INV, 1, unary, lambda a: sc(G.f2_inv(a), R2))]
    packed = pack_fq2(S)
    lanes = 0
    for name, op, nargs, idx, want_fn in cases:
        ia = np.array(idx, dtype=np.int64)
        cols = [packed[ia[:, k]] for k in range(nargs)]
        operands = lambda i: [S[j] for j in idx[i]]
        out = run_op(probe, "pc_probe_fq2", (C.c_int(op),), 24, cols)
        got = list(zip(unpack(out[:, :12]), unpack(out[:, 12:])))
        expect("fq2 " + name, got, [want_fn(*operands(i)) for i in range(len(idx))], lambda i: [str(x) for x in operands(i)])
        if host is not probe:
            same_words("fq2 " + name, out, run_op(host, "pc_probe_fq2", (C.c_int(op),), 24, cols))
        lanes += len(idx)
    return lanes


# ---- groups ------------------------------------------------------------------------------------------------------------------------

class Grp:
    """one group: G1 of a curve (coordinates are integers) or G2 of BLS12-381 (pairs); coordinates cross the probe in Montgomery form"""

    def __init__(self, name):
        self.name, self.g2 = name, name.endswith("_g2")
        self.curve = name[:-3] if self.g2 else name
        self.f = Field(R.CURVES[self.curve]["fq"])
        self.FN = self.f.N * (2 if self.g2 else 1)
        self.entry = "pc_probe_curve_" + name
        self.lazy = self.f.lazy and not self.g2

    def add(self, A, B):
        return G.add(A, B) if self.g2 else R.ec_add(self.curve, A, B)

    def neg(self, A):
        return G.neg(A) if self.g2 else R.ec_neg(self.curve, A)

    def points(self, n):
        g = G.generator() if self.g2 else R.generator(self.curve)
        out = [g]
        while len(out) < n:
            out.append(self.add(out[-1], g))
        return out

    def cmul(self, a, b):
        return G.f2_mul(a, b) if self.g2 else a * b % self.f.p

    def cinv(self, a):
        return G.f2_inv(a) if self.g2 else pow(a, -1, self.f.p)

    def enc(self, c):
        """a coordinate -> its words, Montgomery form"""
        f = self.f
        return pack([x * f.R % f.p for x in (c if self.g2 else (c,))], f.N).reshape(-1)

    def dec(self, w):
        f = self.f
        v = [x * f.Ri % f.p for x in unpack(w.reshape(-1, f.N))]
        return tuple(v) if self.g2 else v[0]

    def zero(self):
        return (0, 0) if self.g2 else 0

    def one(self):
        return (1, 0) if self.g2 else 1

    def affine_words(self, A):
        if A is None:
            return np.zeros(2 * self.FN, dtype=np.uint32)
        return np.concatenate([self.enc(A[0]), self.enc(A[1])])

    def xyzz_words(self, A, lam=None):
        """the point as X | Y | ZZ | ZZZ; lam: the representative (x lam^2, y lam^3, lam^2, lam^3)"""
        if A is None:
            return np.zeros(4 * self.FN, dtype=np.uint32)
        l1 = self.one() if lam is None else lam
        l2 = self.cmul(l1, l1)
        l3 = self.cmul(l2, l1)
        return np.concatenate([self.enc(self.cmul(A[0], l2)), self.enc(self.cmul(A[1], l3)), self.enc(l2), self.enc(l3)])

    def affine_of_xyzz(self, w):
        """the point a row of XYZZ words stands for (any representative, lazily reduced ones included); checks ZZ^3 = ZZZ^2"""
        FN = self.FN
        X, Y, ZZ, ZZZ = (self.dec(w[k * FN:(k + 1) * FN]) for k in range(4))
        if ZZ == self.zero():
            return None
        assert self.cmul(self.cmul(ZZ, ZZ), ZZ) == self.cmul(ZZZ, ZZZ)
        return (self.cmul(X, self.cinv(ZZ)), self.cmul(Y, self.cinv(ZZZ)))

    def affine_of_words(self, w):
        FN = self.FN
        if not w.any():
            return None
        return (self.dec(w[:FN]), self.dec(w[FN:2 * FN]))

    def lam(self, rnd):
        return (rnd.randrange(1, self.f.p), rnd.randrange(self.f.p)) if self.g2 else rnd.randrange(1, self.f.p)


def run_curve(probe, g, op, Pw, Qw=None, flags=None):
    """Pw, Qw: n x (4 FN) XYZZ words (an affine operand in the first 2 FN words of Qw) -> (raw XYZZ words, affine words)"""
    n, FN = len(Pw), g.FN
    inp = np.zeros((n, 8 * FN + 1), dtype=np.uint32)
    inp[:, :4 * FN] = Pw
    if Qw is not None:
        inp[:, 4 * FN:4 * FN + Qw.shape[1]] = Qw
    if flags is not None:
        inp[:, 8 * FN] = flags
    out = np.zeros((n, 6 * FN), dtype=np.uint32)
    probe.call(g.entry, C.c_int(op), C.c_size_t(n), p32(inp), p32(out))
    return out[:, :4 * FN].copy(), out[:, 4 * FN:].copy()


def lifted(host, g, A):
    """a representative with a non-trivial ZZ as tests/emu builds it: 2 A + (-A) through dbl and the mixed addition"""
    if A is None:
        return g.xyzz_words(None)
    d, _ = run_curve(host, g, C_DBL, g.xyzz_words(A)[None, :])
    r, _ = run_curve(host, g, C_ADD_AFFINE, d, g.affine_words(g.neg(A))[None, :])
    return r[0]


CURVE_GROUPS = ["add_affine", "add", "dbl", "add_affine_lz"]


def check_curve(probe, host, gname, group):
    g = Grp(gname)
    FN = g.FN
    if group == "add_affine_lz" and not g.lazy:
        n_in = np.zeros(8 * FN + 1, dtype=np.uint32)
        assert probe.raw(g.entry, C.c_int(C_ADD_AFFINE_LZ), C.c_size_t(1), p32(n_in), p32(np.zeros(6 * FN, dtype=np.uint32))) == UNSUPPORTED
        return 0
    rnd = random.Random(50)
    pts = g.points(5)
    S = pts + [g.neg(pts[1]), g.neg(pts[3]), None]
    # every point as (x, y, 1, 1), as a representative with random lam, and as 2 A - A built by the code itself
    reps = [(A, g.xyzz_words(A)) for A in S] + [(A, g.xyzz_words(A, g.lam(rnd))) for A in S] + [(A, lifted(host, g, A)) for A in S[:6]]

    def verify(name, raw, aff, want, twin_args):
        for i, w in enumerate(want):
            assert g.affine_of_words(aff[i]) == w, "%s %s: affine result of lane %d" % (gname, name, i)
            assert g.affine_of_xyzz(raw[i]) == w, "%s %s: raw XYZZ of lane %d is another point" % (gname, name, i)
        if host is not probe:
            hraw, haff = run_curve(host, g, *twin_args)
            same_words("%s %s raw XYZZ" % (gname, name), raw, hraw)
            same_words("%s %s affine" % (gname, name), aff, haff)

    if group == "add_affine":
        cases = [(rp, B) for rp in reps for B in S]
        Pw = np.array([rp[1] for rp, _ in cases])
        Qw = np.array([g.affine_words(B) for _, B in cases])
        raw, aff = run_curve(probe, g, C_ADD_AFFINE, Pw, Qw)
        verify("add_affine", raw, aff, [g.add(rp[0], B) for rp, B in cases], (C_ADD_AFFINE, Pw, Qw))
        return len(cases)
    if group == "add":
        cases = [(a, b) for a in reps for b in reps]
        Pw, Qw = np.array([a[1] for a, _ in cases]), np.array([b[1] for _, b in cases])
        raw, aff = run_curve(probe, g, C_ADD, Pw, Qw)
        verify("add", raw, aff, [g.add(a[0], b[0]) for a, b in cases], (C_ADD, Pw, Qw))
        return len(cases)
    if group == "dbl":
        Pw = np.array([rp[1] for rp in reps])
        raw, aff = run_curve(probe, g, C_DBL, Pw)
        verify("dbl", raw, aff, [g.add(rp[0], rp[0]) for rp in reps], (C_DBL, Pw))
        Qw = np.array([g.affine_words(A) for A in S])
        Zw = np.zeros((len(S), 4 * FN), dtype=np.uint32)
        raw, aff = run_curve(probe, g, C_DBL_AFFINE, Zw, Qw)
        verify("dbl_affine", raw, aff, [g.add(A, A) for A in S], (C_DBL_AFFINE, Zw, Qw))
        raw, aff = run_curve(probe, g, C_TO_AFFINE, Pw)
        verify("to_affine", raw, aff, [rp[0] for rp in reps], (C_TO_AFFINE, Pw))
        return 2 * len(reps) + len(S)
    # the lazily reduced mixed addition, both signs.  Stage 1: canonical sums.  Stage 2: the sums stage 1 left behind (coordinates
    # anywhere in [0, 2p)), and the same with p added to every coordinate that is below p (infinity keeps its exact zeros).
    p = g.f.p
    cases = [(rp, B, s) for rp in reps for B in S for s in (0, 1)]
    Pw = np.array([rp[1] for rp, _, _ in cases])
    Qw = np.array([g.affine_words(B) for _, B, _ in cases])
    fl = np.array([s for _, _, s in cases], dtype=np.uint32)
    sign = lambda B, s: g.neg(B) if s else B
    raw1, aff = run_curve(probe, g, C_ADD_AFFINE_LZ, Pw, Qw, fl)
    want1 = [g.add(rp[0], sign(B, s)) for rp, B, s in cases]
    verify("add_affine_lz", raw1, aff, want1, (C_ADD_AFFINE_LZ, Pw, Qw, fl))
    assert all(v < 2 * p for v in unpack(raw1.reshape(-1, g.f.N))), "a lazily reduced coordinate is not below 2p"

    def plus_p(row):
        if not row[2 * FN:3 * FN].any():
            return row
        return pack([v + p if v < p else v for v in unpack(row.reshape(4, FN))], FN).reshape(-1)
    sums = [(want1[i], raw1[i]) for i in range(0, len(cases), 3)] + [(want1[i], plus_p(raw1[i])) for i in range(1, len(cases), 3)]
    cases2 = [(sm, B, s) for sm in sums for B in (S[0], S[2], S[5], None) for s in (0, 1)]
    Pw = np.array([sm[1] for sm, _, _ in cases2])
    Qw = np.array([g.affine_words(B) for _, B, _ in cases2])
    fl = np.array([s for _, _, s in cases2], dtype=np.uint32)
    raw2, aff = run_curve(probe, g, C_ADD_AFFINE_LZ, Pw, Qw, fl)
    verify("add_affine_lz on lazy sums", raw2, aff, [g.add(sm[0], sign(B, s)) for sm, B, s in cases2], (C_ADD_AFFINE_LZ, Pw, Qw, fl))
    assert all(v < 2 * p for v in unpack(raw2.reshape(-1, g.f.N)))
    return len(cases) + len(cases2)


# ---- the radix-2^30 running sum: chains ----------------------------------------------------------------------------------------------

NEG = 1 << 31
CHAIN_SPECIAL = {
    "infinite sum, infinite base": [0, 0],
    "infinite base on a finite sum": [3, 0, 0 | NEG, 4],
    "doubling": [5, 5, 7],
    "doubling of a negated digit": [5 | NEG, 5 | NEG, 9],
    "P + (-P), then on from infinity": [6, 6 | NEG, 2, 3],
    "P + (-P)": [6, 6 | NEG],
    "(-P) + P": [6 | NEG, 6, 2 | NEG],
    "doubling deeper in a chain": [1, 2, 3, 6, 12, 24, 48],            # 1 + 2 = 3: + 3 doubles, + 6 doubles, ...
    "cancelling deeper in a chain": [1, 2, 3 | NEG, 5, 5],
    "negated digit": [9 | NEG, 4, 17 | NEG],
}
CHAIN_STEPS = 200


def chain_lists():
    """the special-case lists and three random 200-step lists (entry 0: the infinite base; signed digits), interleaved so that the
    long lists sit between short ones: neighbouring lanes of the one launch take different branches"""
    lists = list(CHAIN_SPECIAL.items())
    for seed in (1, 2, 3):
        rnd = random.Random(seed)
        lists.insert(3 * seed, ("random %d" % seed, [rnd.randrange(64) | (NEG if rnd.random() < 0.5 else 0) for _ in range(CHAIN_STEPS)]))
    return lists


def run_chain(probe, lists, table):
    inp = np.zeros((len(lists), 1 + CHAIN_STEPS), dtype=np.uint32)
    for i, (_, idx) in enumerate(lists):
        inp[i, 0] = len(idx)
        inp[i, 1:1 + len(idx)] = idx
    out = np.zeros((len(lists), 2 + 4 * 48), dtype=np.uint32)
    probe.call("pc_probe_chain30", C.c_size_t(len(lists)), C.c_uint32(CHAIN_STEPS), p32(inp), p32(table), p32(out))
    return out


def check_chain30(probe, host):
    g = Grp("bls12_381")
    p = g.f.p
    pts = [None] + g.points(63)
    table = np.array([g.affine_words(A) for A in pts]).reshape(-1)
    lists = chain_lists()
    out = run_chain(probe, lists, table)
    for (name, idx), row in zip(lists, out):
        want = None
        for e in idx:
            A = pts[e & 63]
            want = g.add(want, g.neg(A) if e & NEG else A)
        raw, c30, clz, cc = (row[2 + 48 * k:2 + 48 * (k + 1)] for k in range(4))
        assert row[0] == 0, "%s: %d steps broke the class invariant or left the lazily reduced sum" % (name, row[0])
        assert all(v < 2 * p for v in unpack(raw.reshape(4, 12))) and all(v < p for v in unpack(c30.reshape(4, 12))), name
        assert (c30 == clz).all() or (want is None and not c30[24:36].any() and not clz[24:36].any()), name
        for w in (raw, c30, clz, cc):
            assert g.affine_of_xyzz(w) == want, name
    if host is not probe:
        same_words("chain30 (bad steps, hash of every step's to32() words, final sums)", out, run_chain(host, lists, table))
    return len(lists)


# ---- the two-lane addition -----------------------------------------------------------------------------------------------------------

HALF_KINDS = ["generic", "doubling", "P + (-P)", "first infinite", "second infinite", "both infinite"]


def half_add_cases(host, g):
    """7 waves of 32 lane pairs: one with pairs of every kind interleaved, then one per kind; every kind with trivial and non-trivial ZZ
    on either side (mode bit 0 / 1: the first / second operand is 2 A - A instead of A)"""
    pts = g.points(9)
    rep = {}

    def operand(A, twist):
        k = (A, twist)
        if k not in rep:
            rep[k] = lifted(host, g, A) if twist else g.xyzz_words(A)
        return rep[k]

    def pair(kind, i, mode):
        A, B = pts[i % 8], pts[(i % 8 + 1 + (i // 8) % 7) % 8]                 # B != A, and A + B stays a generic sum
        A, B = {"generic": (A, B), "doubling": (A, A), "P + (-P)": (A, g.neg(A)), "first infinite": (None, B), "second infinite": (A, None),
                "both infinite": (None, None)}[kind]
        return kind, A, B, operand(A, mode & 1), operand(B, mode & 2)
    cases = [pair(HALF_KINDS[k % 6], k, (k // 6) % 4) for k in range(24)] + [pair("generic", k, k % 4) for k in range(24, 32)]
    for kind in HALF_KINDS:
        cases += [pair(kind, k, k // 8) for k in range(32)]
    return cases


def check_half_add(probe, host, curve):
    g = Grp(curve)
    FN = g.FN
    cases = half_add_cases(host, g)
    inp = np.array([np.concatenate([c[3], c[4]]) for c in cases], dtype=np.uint32)

    def run(pr):
        out = np.zeros((len(cases), 8 * FN), dtype=np.uint32)
        pr.call("pc_probe_half_add_" + curve, C.c_size_t(len(cases)), p32(inp), p32(out))
        return out
    out = run(probe)
    for i, (kind, A, B, _, _) in enumerate(cases):
        assert (out[i, :4 * FN] == out[i, 4 * FN:]).all(), "%s pair %d (%s): the lane pair's XYZZ words differ from XyzzD::add's" % (curve, i, kind)
        assert g.affine_of_xyzz(out[i, :4 * FN]) == g.add(A, B), "%s pair %d (%s)" % (curve, i, kind)
    if host is not probe:
        same_words("%s half_add" % curve, out, run(host))
    return len(cases)
