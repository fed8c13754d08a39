"""G1 keys with KNOWN discrete logarithms and BOTH signs, and the scalar layouts that make an MSM over them cancel inside the pipeline.

Pool: per curve 8 points Q_i = k_i G (G the Python reference's generator; the k_i seeded, odd, pairwise different and k_i != r - k_j,
so Q_i != +-Q_j).  A key is a list of logarithms e_j in {+k_i, -k_i, 0} (0: the all-zero words of the point at infinity) and the
Montgomery words of the points e_j G:

  signed(n)              K[j] = (-1)^j Q[(j // 2) mod 8]: neighbours are P, -P
  signed(n, holes=True)  the same with K[j] = infinity where j mod 64 == 11
  unsigned(n)            K[j] = Q[(j // 2) mod 8]
  one_base(n)            K[j] = Q[0]
  halves(n)              K[j] = Q[j mod 8] for j < n / 2, K[j + n / 2] = -K[j]

Whatever the MSM does, its result over such a key is (sum_j s_j e_j mod r) G: Python integers and ONE scalar multiplication
(`expected`), all-zero words when the sum is 0 mod r.  Neither the device nor the oracle's bucket method has a part in it.

`layouts` makes the scalar sets.  A pair is two KEY positions 2t, 2t + 1, so a layout is laid against the key window it will meet
(`start`: the base offset of the call): position start + i of the key gets scalar i.  An entry whose partner is not there -- the
window begins at an odd position or ends at an even one, or the partner is a hole -- gets the scalar 0, so that a layout that is said
to cancel does cancel under every offset and with holes in the key.  (A hole itself keeps its scalar: a non-zero scalar on the point
at infinity is part of what is tested.)
"""
import random

import numpy as np

import oracle_lib as O

CURVES = ["bls12_381", "bn254", "pallas", "bls12_377"]
POOL = 8
HOLE_PERIOD, HOLE_AT = 64, 11
_pools = {}


def modulus(curve):
    ref = O.ref(curve)
    return ref.FIELDS[ref.CURVES[curve]["fr"]]["p"]


def limbs(vals, n64=4):
    """integers -> (len, n64) uint64, little-endian limbs"""
    return np.frombuffer(b"".join(int(v).to_bytes(8 * n64, "little") for v in vals), dtype=np.uint64).reshape(len(vals), n64).copy()


def pool(curve):
    """(k_0 .. k_7, the 17 x 2N words of [+Q_0 .. +Q_7, -Q_0 .. -Q_7, infinity])"""
    if curve not in _pools:
        ref, r = O.ref(curve), modulus(curve)
        rnd = random.Random(0x51C0ED + O.CURVES[curve])
        ks = []
        while len(ks) < POOL:
            k = rnd.randrange(3, r) | 1
            if k < r and all(k != q and k != r - q for q in ks):
                ks.append(k)
        G = ref.generator(curve)
        pts = [ref.ec_mul(curve, k, G) for k in ks]
        assert all(ref.on_curve(curve, P) for P in pts)
        words = O.points_to_array(curve, pts + [ref.ec_neg(curve, P) for P in pts] + [None])
        _pools[curve] = (ks, words)
    return _pools[curve]


class Key:
    """idx[j]: the row of the pool's word table (i: +Q_i, 8 + i: -Q_i, 16: infinity)"""

    def __init__(self, curve, idx):
        self.curve, self.idx = curve, np.asarray(idx, dtype=np.intp)
        ks, words = pool(curve)
        self.bases = np.ascontiguousarray(words[self.idx])
        table = list(ks) + [-k for k in ks] + [0]
        self.logs = [table[i] for i in self.idx]

    def __len__(self):
        return len(self.logs)

    def is_hole(self, j):
        return self.idx[j] == 2 * POOL


def signed(curve, n, holes=False):
    j = np.arange(n)
    idx = (j // 2) % POOL + POOL * (j & 1)
    if holes:
        idx[j % HOLE_PERIOD == HOLE_AT] = 2 * POOL
    return Key(curve, idx)


def unsigned(curve, n):
    return Key(curve, (np.arange(n) // 2) % POOL)


def one_base(curve, n):
    return Key(curve, np.zeros(n, dtype=np.intp))


def halves(curve, n):
    assert n % 2 == 0
    first = np.arange(n // 2) % POOL
    return Key(curve, np.concatenate([first, first + POOL]))


def expected(key, scalars, off=0):
    """the MSM of `scalars` (integers) over key[off:]: (sum s_j e_j mod r) G as the ABI's affine Montgomery words; all zero = infinity"""
    ref, r = O.ref(key.curve), modulus(key.curve)
    t = sum(s * e for s, e in zip(scalars, key.logs[off:])) % r
    return O.points_to_array(key.curve, [ref.ec_mul(key.curve, t, ref.generator(key.curve)) if t else None])[0]


def _paired(start, n, holes):
    """per scalar index i: the pair number (start + i) // 2 of its key position, or -1 where the partner is missing"""
    out = []
    for i in range(n):
        j = start + i
        p = j ^ 1
        there = start <= p < start + n and not (holes and p % HOLE_PERIOD == HOLE_AT)
        out.append(j // 2 if there else -1)
    return out


def _first_live(start, n, holes, at):
    """the first index >= at whose key position is no hole (a changed scalar on a hole would change nothing)"""
    while holes and (start + at) % HOLE_PERIOD == HOLE_AT:
        at += 1
    assert at < n
    return at


def const(curve, n, seed, start=0, holes=False, k=None):
    """ONE scalar k on every paired entry: on a signed key every bucket of every window holds as many P as -P"""
    if k is None:
        k = random.Random(seed).randrange(1, modulus(curve))
    return [k if p >= 0 else 0 for p in _paired(start, n, holes)]


LAYOUTS = ("const", "pairwise", "pairwise_few", "all_but_one", "opposite_scalars")


def layout(name, curve, n, seed, start=0, holes=False):
    """one scalar set of `layouts` (the same values: every set draws from its own generator)"""
    r = modulus(curve)
    if name == "const":
        return const(curve, n, seed ^ 0xC0, start, holes)
    pair = _paired(start, n, holes)
    if name == "pairwise_few":
        rnd = random.Random(seed ^ 0xFE3)
        few = [rnd.randrange(1, r) for _ in range(5)]
        return [few[p % 5] if p >= 0 else 0 for p in pair]
    rnd = random.Random(seed)
    vals = {}
    pairwise = [(vals.get(p) or vals.setdefault(p, rnd.randrange(1, r))) if p >= 0 else 0 for p in pair]
    if name == "pairwise":
        return pairwise
    if name == "all_but_one":
        at = _first_live(start, n, holes, n // 3)
        pairwise[at] = (pairwise[at] + rnd.randrange(1, r - 1)) % r or 1
        return pairwise
    assert name == "opposite_scalars", name
    return [0 if p < 0 else (pairwise[i] if (start + i) % 2 == 0 else r - pairwise[i]) for i, p in enumerate(pair)]


def layouts(curve, n, seed, start=0, holes=False):
    """name -> list of n canonical scalars.  On signed(.., holes) from position `start`: const, pairwise, pairwise_few sum to infinity,
    all_but_one (pairwise with ONE scalar replaced) to a known point; on unsigned(..): opposite_scalars (s[2t + 1] = r - s[2t]) sums to
    infinity, but only behind the buckets; const on one_base(..) makes every partial sum of a bucket equal."""
    return {name: layout(name, curve, n, seed, start, holes) for name in LAYOUTS}


def all_but_one_on_const(curve, n, seed, start=0, holes=False):
    """const with ONE scalar changed: every entry but one sits in one bucket per window"""
    s = const(curve, n, seed, start, holes)
    at = _first_live(start, n, holes, n // 3)
    s[at] = (s[at] + 12345) % modulus(curve) or 1
    return s


def rand_scalars(curve, n, seed):
    rnd, r = random.Random(seed), modulus(curve)
    return [rnd.randrange(r) for _ in range(n)]


def mont(curve, vals):
    """integers -> Montgomery-form scalar words"""
    r = modulus(curve)
    return limbs([v * (1 << 256) % r for v in vals])
