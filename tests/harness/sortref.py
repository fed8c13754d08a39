"""Reference for the contract of the MSM's bucket sort (HipBackend::sort_entries), written from the description of the recoding in
csrc/msm.hpp and importing nothing of the code under test.

The sort takes n canonical scalars and a call geometry and returns a CSR structure over NB = W * 2^(c-1) buckets: `offsets[NB + 1]` and
`entries[offsets[NB]]`.  Every scalar is recoded in signed radix 2^c -- windows of c bits from the bottom, a digit above 2^(c-1)
becomes digit - 2^c with a carry into the next window, so digits lie in [-(2^(c-1) - 1), 2^(c-1)]; the top window is zero-extended and
takes the last carry.  A non-zero digit of magnitude `mag` in window w of scalar i goes to bucket `set * 2^(c-1) + mag - 1` as the entry
word `base | neg << 31`:

  mode      bucket set                 base index
  plain     w                          base_off + i
  table     0                          w * tbl_stride + base_off + i
  many      i // m_sub                 w * tbl_stride + base_off + i % m_sub
  GLV       the half h (with many: 2 * (i // m_sub) + h)       as table / many

In the GLV modes the scalar is first split into k = k1 + k2 lambda (mod r) with |k_h| < 2^130; the magnitudes |k_h| are recoded over
130 // c + 1 windows each and a negative half flips the sign of its digits.

recode() is vectorised over the 32-bit limbs; recode_int() is the same over Python integers, one scalar at a time, and checks it.
check_sort() runs the three exact checks of a sort's output: CSR, content, reconstruction."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CURVES = {"bls12_381": 0, "bn254": 1, "pallas": 2, "bls12_377": 3}
FR_BITS = {"bls12_381": 255, "bn254": 254, "pallas": 255, "bls12_377": 253}
FR_WORDS = 8
HALF_BITS, HALF_WORDS = 130, 5
_gen = None


def gen_constants():
    """tools/gen_constants.py: the scalar moduli, lambda and the device's split of a scalar (glv_decompose_like_device)"""
    global _gen
    if _gen is None:
        spec = importlib.util.spec_from_file_location("_gen_constants_sortref", os.path.join(ROOT, "tools", "gen_constants.py"))
        _gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_gen)
    return _gen


_glv = {}


def glv(curve):
    if curve not in _glv:
        _glv[curve] = gen_constants().glv_constants(curve)
    return _glv[curve]


def modulus(curve):
    G = gen_constants()
    return G.R.FIELDS[G.R.CURVES[curve]["fr"]]["p"]


class Geom:
    """one call of the sort: tbl_stride == 0 plain; else table mode, with m_sub many-MSM mode, with glv the two halves' bucket sets"""

    def __init__(self, curve, n, c, tbl_stride=0, m_sub=0, glv=0, base_off=0):
        assert (not glv and not m_sub) or tbl_stride
        self.curve, self.n, self.c, self.tbl_stride, self.m_sub, self.glv, self.base_off = curve, n, c, tbl_stride, m_sub, glv, base_off
        self.bits = FR_BITS[curve]
        self.sets = 2 if glv else 1
        self.windows = (HALF_BITS if glv else self.bits) // c + 1
        self.Wd = self.windows * self.sets
        self.subs = n // m_sub if m_sub else 0
        self.W = self.subs * self.sets if m_sub else self.sets if tbl_stride else self.Wd
        self.nb_win = 1 << (c - 1)
        self.NB = self.W * self.nb_win

    def __repr__(self):
        return "Geom(%s, n=%d, c=%d, tbl_stride=%d, m_sub=%d, glv=%d, base_off=%d)" % (self.curve, self.n, self.c, self.tbl_stride, self.m_sub, self.glv, self.base_off)


# ---- words <-> integers ------------------------------------------------------------------------------------------------------------

def to_limbs(vals, words=FR_WORDS):
    return np.frombuffer(b"".join(int(v).to_bytes(4 * words, "little") for v in vals), dtype=np.uint32).reshape(len(vals), words).copy()


def to_ints(limbs):
    w = limbs.shape[1]
    raw = np.ascontiguousarray(limbs, dtype=np.uint32).tobytes()
    return [int.from_bytes(raw[4 * w * i:4 * w * (i + 1)], "little") for i in range(limbs.shape[0])]


# ---- the recoding ------------------------------------------------------------------------------------------------------------------

def recode_int(k, c, windows):
    """signed digits of the non-negative integer k, lowest window first"""
    half, out, carry = 1 << (c - 1), [], 0
    for w in range(windows):
        raw = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if raw > half else 0
        out.append(raw - (carry << c))
    assert carry == 0 and k >> (c * windows) == 0, "the scalar does not fit its windows"
    return out


def raw_windows(limbs, c, windows):
    """(n, windows) unsigned c-bit windows of little-endian 32-bit limbs, zero-extended"""
    n, L = limbs.shape
    ext = np.concatenate([limbs.astype(np.uint64), np.zeros((n, 2), dtype=np.uint64)], axis=1)
    out = np.zeros((n, windows), dtype=np.int64)
    mask = np.uint64((1 << c) - 1)
    for w in range(windows):
        word, b = (c * w) >> 5, (c * w) & 31
        if word >= L:
            break
        v = ext[:, word] | (ext[:, word + 1] << np.uint64(32))
        out[:, w] = ((v >> np.uint64(b)) & mask).astype(np.int64)
    return out


def recode(limbs, c, windows):
    """(n, windows) signed digits (int64) of the scalars in `limbs`"""
    d = raw_windows(limbs, c, windows)
    half = 1 << (c - 1)
    carry = np.zeros(limbs.shape[0], dtype=np.int64)
    for w in range(windows):
        raw = d[:, w] + carry
        carry = (raw > half).astype(np.int64)
        d[:, w] = raw - (carry << c)
    assert not carry.any(), "a scalar does not fit its windows"
    return d


def unique_rows(a):
    """(the distinct rows of a, the index of every row among them): grouped by a 64-bit mix of the row, the groups then compared word
    for word (two distinct rows under one mix send this to numpy's row sort)"""
    a = np.ascontiguousarray(a)
    mult = np.random.RandomState(64).randint(0, 1 << 63, size=a.shape[1], dtype=np.uint64) | np.uint64(1)
    mix = (a.astype(np.uint64) * mult).sum(axis=1, dtype=np.uint64)
    _, first, inv = np.unique(mix, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    if not np.array_equal(a[first][inv], a):
        uniq, inv = np.unique(a, axis=0, return_inverse=True)
        return uniq, np.asarray(inv).reshape(-1)
    return a[first], inv


def glv_halves(curve, canon):
    """the device's split of every scalar: (n, 2, 5) magnitudes and (n, 2) signs (1 = negative); one Python split per distinct scalar"""
    G, gc = gen_constants(), glv(curve)
    uniq, inv = unique_rows(canon)
    mags, negs = [], []
    for k in to_ints(uniq):
        k1, k2 = G.glv_decompose_like_device(gc, k)
        assert abs(k1) < 1 << HALF_BITS and abs(k2) < 1 << HALF_BITS
        mags += [abs(k1), abs(k2)]
        negs += [int(k1 < 0), int(k2 < 0)]
    mags = to_limbs(mags, HALF_WORDS).reshape(len(uniq), 2, HALF_WORDS)
    negs = np.array(negs, dtype=np.int64).reshape(len(uniq), 2)
    return mags[inv], negs[inv]


def signed_digits(g, canon):
    """(n, sets, windows) signed digits of the call's scalars: the scalar's own, or those of its two halves with the halves' signs"""
    assert canon.shape == (g.n, FR_WORDS)
    assert below_modulus(g.curve, canon).all(), "a scalar is not below r"
    if not g.glv:
        return recode(canon, g.c, g.windows)[:, None, :]
    mags, negs = glv_halves(g.curve, canon)
    d = np.stack([recode(np.ascontiguousarray(mags[:, h]), g.c, g.windows) for h in range(2)], axis=1)
    return d * (1 - 2 * negs)[:, :, None]


def ref_sort(g, canon):
    """(keys, entries) of every non-zero digit, in no particular order"""
    d = signed_digits(g, canon)
    i, h, w = np.nonzero(d)
    v = d[i, h, w]
    mag, neg = np.abs(v), (v < 0).astype(np.int64)
    sub, j = (i // g.m_sub, i % g.m_sub) if g.m_sub else (np.zeros_like(i), i)
    bset = sub * g.sets + h if g.m_sub else h if g.tbl_stride else w
    keys = bset * g.nb_win + mag - 1
    base = g.base_off + j + (w * g.tbl_stride if g.tbl_stride else 0)
    assert base.size == 0 or base.max() < 1 << 31
    return keys.astype(np.int64), (base | (neg << 31)).astype(np.uint32)


def ref_sort_int(g, ints):
    """the same, one Python integer at a time (plain, table and many modes): a sorted list of (key, entry)"""
    assert not g.glv
    out = []
    for i, k in enumerate(ints):
        sub, j = (i // g.m_sub, i % g.m_sub) if g.m_sub else (0, i)
        for w, dgt in enumerate(recode_int(k, g.c, g.windows)):
            if dgt:
                bset = sub if g.m_sub else 0 if g.tbl_stride else w
                base = g.base_off + j + (w * g.tbl_stride if g.tbl_stride else 0)
                out.append((bset * g.nb_win + abs(dgt) - 1, base | (int(dgt < 0) << 31)))
    return sorted(out)


# ---- the checks --------------------------------------------------------------------------------------------------------------------

def _pairs(keys, entries):
    return np.sort((keys.astype(np.uint64) << np.uint64(32)) | entries.astype(np.uint64))


def digits_to_limbs(d, c, words):
    """(n, windows) signed digits -> sign (1 = the sum is negative) and the magnitude's little-endian limbs; None where the magnitude
    does not fit `words` limbs"""
    n, windows = d.shape
    top = np.zeros(n, dtype=np.int64)
    for w in range(windows):                       # the sign of the sum is the sign of its highest non-zero digit (|digit| <= 2^(c-1))
        top = np.where(d[:, w] != 0, d[:, w], top)
    neg = (top < 0).astype(np.int64)
    d = d * (1 - 2 * neg)[:, None]
    limbs = np.zeros((n, words + 2), dtype=np.uint64)
    borrow = np.zeros(n, dtype=np.int64)
    for w in range(windows):
        u = d[:, w] + borrow
        borrow = -(u < 0).astype(np.int64)
        u = (u - (borrow << c)).astype(np.uint64)          # back to the unsigned window in [0, 2^c)
        word, b = (c * w) >> 5, (c * w) & 31
        if word >= words:
            if u.any():
                return None
            continue
        v = u << np.uint64(b)
        limbs[:, word] |= v & np.uint64(0xffffffff)
        limbs[:, word + 1] |= v >> np.uint64(32)
    if borrow.any() or limbs[:, words:].any():
        return None
    return neg, limbs[:, :words].astype(np.uint32)


def check_sort(g, canon, offsets, entries):
    """offsets: NB + 1 words, entries: n * Wd words as the sort left them.  Returns the number of entries."""
    what = repr(g)
    assert offsets.shape == (g.NB + 1,) and entries.shape == (g.n * g.Wd,)
    rkeys, rent = ref_sort(g, canon)
    M = int(offsets[-1])
    # -- CSR: offsets is the exclusive prefix sum of the reference's bucket counts, empty buckets included
    assert offsets[0] == 0, "%s: offsets[0] = %d" % (what, offsets[0])
    assert M == len(rkeys), "%s: offsets[NB] = %d, the scalars have %d non-zero digits" % (what, M, len(rkeys))
    step = np.diff(offsets)                          # (uint32: a decreasing step wraps to a huge count and fails below)
    nz = np.flatnonzero(step)
    if g.NB <= 1 << 24:
        counts = np.bincount(rkeys, minlength=g.NB)
        uk = np.flatnonzero(counts)
        uc = counts[uk]
    else:
        uk, uc = np.unique(rkeys, return_counts=True)
    assert np.array_equal(nz, uk) and np.array_equal(step[nz].astype(np.int64), uc), "%s: bucket sizes differ from the reference" % what
    # -- content: every bucket's entries as a sorted multiset
    used = entries[:M]
    pos_key = np.repeat(nz, step[nz])                # the bucket of every position (the sizes sum to M: checked above)
    got, want = _pairs(pos_key, used), _pairs(rkeys, rent)
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: sorted (bucket, entry) pair %d is (%d, %#x), reference (%d, %#x)" % (
            what, k, got[k] >> 32, got[k] & 0xffffffff, want[k] >> 32, want[k] & 0xffffffff))
    assert (entries[M:] == 0xffffffff).all(), "%s: the sort wrote behind offsets[NB]" % what
    # -- reconstruction: from the output alone
    reconstruct(g, canon, pos_key, used)
    return M


def reconstruct(g, canon, pos_key, used):
    """every (scalar, set, window) at most once, and the digits sum to the scalar (GLV: to halves with k1 + lambda k2 = k mod r)"""
    what = repr(g)
    base, neg = (used & np.uint32(0x7fffffff)).astype(np.int64), (used >> np.uint32(31)).astype(np.int64)
    bset, mag = pos_key // g.nb_win, pos_key % g.nb_win + 1
    if g.tbl_stride:
        w, j = base // g.tbl_stride, base % g.tbl_stride - g.base_off
        sub, h = (bset // g.sets, bset % g.sets) if g.m_sub else (np.zeros_like(bset), bset)
        i = sub * g.m_sub + j if g.m_sub else j
        assert ((j >= 0) & (j < (g.m_sub or g.n))).all(), "%s: a base index outside the call's bases" % what
    else:
        w, i, h = bset, base - g.base_off, np.zeros_like(bset)
    assert ((i >= 0) & (i < g.n) & (w < g.windows) & (h < g.sets)).all(), "%s: an entry names no digit of the call" % what
    slot = (i * g.sets + h) * g.windows + w
    assert np.bincount(slot, minlength=1).max(initial=0) <= 1, "%s: a (scalar, set, window) occurs twice" % what
    d = np.zeros(g.n * g.sets * g.windows, dtype=np.int64)
    d[slot] = mag * (1 - 2 * neg)
    d = d.reshape(g.n * g.sets, g.windows)
    if not g.glv:
        r = digits_to_limbs(d, g.c, FR_WORDS)
        assert r is not None, "%s: a digit sum leaves 256 bits" % what
        sneg, limbs = r
        assert not (sneg & limbs.any(axis=1)).any(), "%s: a digit sum is negative" % what
        assert np.array_equal(limbs, canon), "%s: the digits of scalar %d do not sum to it" % (what, int(np.flatnonzero((limbs != canon).any(axis=1))[0]))
        return
    r = digits_to_limbs(d, g.c, HALF_WORDS)
    assert r is not None, "%s: a half leaves 160 bits" % what
    sneg, limbs = r
    rows = np.concatenate([canon, limbs.reshape(g.n, 2 * HALF_WORDS), sneg.reshape(g.n, 2).astype(np.uint32)], axis=1)
    rows = unique_rows(rows)[0]
    assert len(rows) == len(unique_rows(canon)[0]), "%s: equal scalars were split differently" % what
    lam, rmod = glv(g.curve)["lam"], modulus(g.curve)
    ks, h1, h2 = to_ints(rows[:, :FR_WORDS]), to_ints(rows[:, FR_WORDS:FR_WORDS + HALF_WORDS]), to_ints(rows[:, FR_WORDS + HALF_WORDS:FR_WORDS + 2 * HALF_WORDS])
    for k, a, b, s in zip(ks, h1, h2, rows[:, -2:]):
        assert a < 1 << HALF_BITS and b < 1 << HALF_BITS, "%s: a half of %#x has more than 130 bits" % (what, k)
        k1, k2 = (-a if s[0] else a), (-b if s[1] else b)
        assert (k1 + lam * k2 - k) % rmod == 0, "%s: the halves of %#x do not recombine" % (what, k)


# ---- scalar sets -------------------------------------------------------------------------------------------------------------------

def pattern(digit, c, bits, top):
    """every whole window below bit `bits` equal to `digit`, as long as the value stays below `top`"""
    v, w = 0, 0
    while c * (w + 1) <= bits and v + (digit << (c * w)) < top:
        v += digit << (c * w)
        w += 1
    return v


def edge_scalars(curve, c, glv_mode=False):
    """0, 1, r - 1, r - 2; every window digit 2^(c-1) (no carry, last bucket) and 2^(c-1) + 1 (a carry through every window into the
    top one); 2^k and 2^k - 1 for every k; scalars whose top window is empty; in GLV mode also k1 + lambda k2 for such halves"""
    r, bits = modulus(curve), FR_BITS[curve]
    half = 1 << (c - 1)
    vals = [0, 1, r - 1, r - 2, pattern(half, c, bits, r), pattern(half + 1, c, bits, r), pattern((1 << c) - 1, c, bits, r)]
    for k in range(bits + 1):
        vals += [v for v in ((1 << k), (1 << k) - 1) if v < r]
    top_start = c * (bits // c)                         # first bit of the top window
    vals += [v for v in ((1 << top_start) - 1, (1 << (top_start - 1)) + 12345, pattern(half + 1, c, top_start - c, r)) if v < r]
    if glv_mode:
        lam = glv(curve)["lam"]
        hs = [pattern(half, c, HALF_BITS - 3, 1 << 127), pattern(half + 1, c, HALF_BITS - 3, 1 << 127), (1 << 127) - 1, 1, 0]
        vals += [(a + s * lam * b) % r for a in hs for b in hs for s in (1, -1)]
    return vals


def below_modulus(curve, limbs):
    """per row: the little-endian limbs are a canonical scalar (below r)"""
    top = limbs[:, ::-1].astype(np.int64) - to_limbs([modulus(curve)], limbs.shape[1])[0, ::-1].astype(np.int64)
    first = np.argmax(top != 0, axis=1)
    return top[np.arange(limbs.shape[0]), first] < 0


def uniform(curve, n, seed, bits=None):
    """n scalars uniform below r (below 2^bits with `bits`), as (n, 8) limbs: rejection sampling on the masked words"""
    rnd = np.random.RandomState(seed)
    nbits = FR_BITS[curve] if bits is None else bits
    mask = to_limbs([(1 << nbits) - 1])[0]
    out = np.zeros((n, FR_WORDS), dtype=np.uint32)
    todo = np.arange(n)
    while todo.size:
        out[todo] = rnd.randint(0, 1 << 32, size=(todo.size, FR_WORDS), dtype=np.uint64).astype(np.uint32) & mask
        todo = todo[~below_modulus(curve, out[todo])]
    return out
