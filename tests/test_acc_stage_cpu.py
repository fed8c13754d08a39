"""CPU suite: the staging policy of the bucket accumulation's prefetched base (csrc/msm.hpp AccumulateBody::chunk, StageRegs;
csrc/msm_coop.hpp StageLds).  tests/emu/emu_acc_stage.cpp steps chunk() for BLS12-381 lane by lane with the register policy and
with a host stand-in of the LDS policy -- an array indexed like the workgroup's exchange tile -- over one sorted entry list: the
buckets, the partial keys, the partial points and each lane's last-run copy must be identical word for word, and every bucket that
the chunks finish must be the oracle's sum of its entries.
(The library is rebuilt when msm.hpp, ec.hpp, fp32.hpp or fp30.hpp is newer than it.)"""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
import pyref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CURVE = "bls12_381"
KEY_INVALID = 0xFFFFFFFF
PW = 48          # words of an XYZZ point
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "emu", "libemu_acc_stage.so")
        srcs = [os.path.join(HERE, "emu", "emu_acc_stage.cpp")] + [
            os.path.join(HERE, "..", "poly_commit_amd", "csrc", f) for f in ("msm.hpp", "ec.hpp", "fp32.hpp", "fp30.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _lib = C.CDLL(so)
    return _lib


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def sorted_entries():
    """A few hundred entries sorted by bucket: empty buckets (single ones, a run of them, the first and the last bucket), one-entry
    buckets, a bucket longer than several chunks (transparent lanes), both signs, the point at infinity at the first, a middle and the
    last position of a chunk, a base twice in one bucket with equal signs (doubling) and a base with its negative (sum to infinity)."""
    T = 7
    sizes = [0, 3, 1, 0, 0, 0, 9, 40, 2, 0, 7, 7, 1, 1, 23, 0, 5, 14, 64, 0, 11, 3, 30, 6, 0, 0, 2, 19, 8, 0]
    n_bases = 97
    rng = np.random.RandomState(8)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    M = int(offsets[-1])
    idx = rng.randint(0, n_bases, size=M).astype(np.uint32)
    neg = rng.randint(0, 2, size=M).astype(np.uint32)
    bases = O.gen_bases(CURVE, n_bases)
    bases[5] = 0                                        # the point at infinity
    for pos in (2 * T, 3 * T + 3, 5 * T - 1):           # first, middle, last position of a chunk
        idx[pos] = 5
    a = int(offsets[7])                                 # the 40-entry bucket: a doubling and a cancellation inside it
    idx[a + 4], neg[a + 4] = idx[a + 3], neg[a + 3]
    idx[a + 20], neg[a + 20] = idx[a + 19], 1 - neg[a + 19]
    b = int(offsets[6])                                 # the 9-entry bucket sums to infinity: four cancelling pairs around an infinity
    idx[b:b + 9] = [11, 11, 12, 12, 5, 13, 13, 14, 14]
    neg[b:b + 9] = [0, 1, 1, 0, 0, 0, 1, 1, 0]
    assert any(int(o) % T for o in offsets[1:-1])       # chunk edges inside buckets
    return T, offsets, idx | (neg << 31), bases


def run(policy, T, offsets, entries, bases):
    NB, M = len(offsets) - 1, int(offsets[-1])
    lanes = (M + T - 1) // T + 2                        # two lanes behind the entries: they run no loop
    b32 = np.ascontiguousarray(bases).view(np.uint32)
    buckets = np.zeros(NB * PW, dtype=np.uint32)
    pkeys = np.full(2 * lanes, 0x55555555, dtype=np.uint32)
    ppts = np.full(2 * lanes * PW, 0x77777777, dtype=np.uint32)
    last = np.zeros(lanes * PW, dtype=np.uint32)
    shared = lib().emu_acc_stage_chunks(p32(b32), 24, p32(entries), p32(offsets), NB, T, lanes, policy, p32(buckets), p32(pkeys), p32(ppts),
                                        p32(last))
    assert shared == 0, "two lanes of a workgroup share words of the tile"
    return buckets, pkeys, ppts, last


def test_lds_stage_policy_equals_register_policy_word_for_word():
    T, offsets, entries, bases = sorted_entries()
    regs = run(0, T, offsets, entries, bases)
    tile = run(1, T, offsets, entries, bases)
    for name, a, b in zip(("buckets", "partial keys", "partial points", "last-run copies"), regs, tile):
        assert (a == b).all(), name
    buckets, pkeys = regs[0], regs[1]
    assert (pkeys != KEY_INVALID).any() and (pkeys[-4:] == KEY_INVALID).all()
    # every bucket no chunk edge cuts was finished by its lane: the oracle's sum of its entries (a negative entry has the scalar r - 1)
    r = R.FIELDS["bls12_381_fr"]["p"]
    whole = 0
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if hi > lo and lo // T != (hi - 1) // T:
            continue
        out = np.zeros(24, dtype=np.uint32)
        lib().emu_acc_stage_affine(p32(np.ascontiguousarray(buckets[k * PW:(k + 1) * PW])), p32(out))
        want = np.zeros(12, dtype=np.uint64)
        if hi > lo:
            e = entries[lo:hi]
            sc = O.ints_to_limbs([r - 1 if int(v) >> 31 else 1 for v in e], 4)
            want = O.msm_naive(CURVE, np.ascontiguousarray(bases[(e & 0x7FFFFFFF).astype(np.int64)]), sc)
            whole += 1
        assert (out.view(np.uint64) == want).all(), k
    assert whole >= 5                                   # (a property of the entry list above, not of the code under test)


def test_tile_slots_are_disjoint_and_conflict_free():
    """The slot layout (msm.hpp acc_stage_word): 256 lanes x 6 pieces of four words tile the first 24 KiB exactly once, and
    the 64 lanes of a wave read a piece from 64 consecutive 16-byte cells (no two lanes in one bank group)."""
    words = set()
    for tid in range(256):
        for j in range(6):
            w = lib().emu_acc_stage_word(tid, j)
            assert w % 4 == 0
            words.update(range(w, w + 4))
    assert words == set(range(24 * 256))
    for wave in range(4):
        for j in range(6):
            cells = [lib().emu_acc_stage_word(wave * 64 + l, j) for l in range(64)]              # in lane order: what one LDS-DMA instruction writes
            assert cells == list(range(cells[0], cells[0] + 256, 4))
