"""Key validation on the device (csrc/validate.hpp, abi_validate.hip) against the plain-integer reference tests/harness/swvalidate.py:
the bodies one point per lane through the probe (compared with the reference and, word for word, with the host build), and the C ABI
-- pc_hip_srs_check with planted non-members at the wave and workgroup edges, through windows, under both values of
PC_HIP_SUBGROUP_LADDER; keys of infinities; the cached answer of pc_hip_srs_in_subgroup and where it carries over;
pc_hip_srs_load_serialized_ex; pc_hip_g2_srs_check; the argument errors."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from harness import g2ref as G2
from harness import swvalidate as V

pytestmark = pytest.mark.gpu
S, R = V.S, V.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


# ---- the bodies, one point per lane ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", V.CURVES)
def test_on_curve_body(curve):
    assert V.check_on_curve(V.device_probe(), V.host_probe(), curve) == len(V.on_curve_cases(curve)[0])


@pytest.mark.parametrize("curve", V.CURVES)
def test_plain_ladder_body(curve):
    assert len(V.check_subgroup(V.device_probe(), V.host_probe(), curve, "pc_probe_validate_ladder")) == len(V.adversarial(curve))


@pytest.mark.parametrize("curve", V.BLS12)
def test_fast_body_agrees_with_the_plain_ladder(curve):
    dev, host = V.device_probe(), V.host_probe()
    fast = V.check_subgroup(dev, host, curve, "pc_probe_validate_fast")
    assert np.array_equal(fast, V.check_subgroup(dev, host, curve, "pc_probe_validate_ladder"))


def test_g2_bodies():
    kinds, _, _, sub = V.g2_cases()
    assert V.check_g2(V.device_probe(), V.host_probe()) == len(kinds) + sum(1 for s in sub if s is not None)


def test_tally_body():
    assert V.check_tally(V.device_probe(), V.host_probe()) == 1 + 1 + 64 + 65 + 257 + 257 + 1000 + 1000


# ---- pc_hip_srs_check -------------------------------------------------------------------------------------------------------------------

def _check_key(ctx, curve, words, on, both, at, wins=None):
    """every window of the key (or `wins`) under the three values of `what`, against the reference's per-point flags"""
    key = V.upload_words(ctx, curve, words)
    try:
        member_only = [1 if o == 0 else b for o, b in zip(on, both)]      # the subgroup bit alone is asked about on-curve points only
        for off, cnt in wins or V.windows(len(words), at):
            assert V.query(key, off, cnt, True, True) == V.expect_query(both, off, cnt), (curve, off, cnt, "both")
            assert V.query(key, off, cnt, True, False) == V.expect_query(on, off, cnt), (curve, off, cnt, "on_curve")
            if all(on):
                assert V.query(key, off, cnt, False, True) == V.expect_query(member_only, off, cnt), (curve, off, cnt, "subgroup")
    finally:
        key.free()


@pytest.mark.parametrize("n", V.SIZES)
@pytest.mark.parametrize("curve", V.BLS12)
def test_planted_non_members(ctx, curve, n):
    """non-members at index 0, n - 1, 63, 64, 255 and 256 where they exist, one at a time, then all at once -- with every other kind of
    non-member beside them where the key has room -- and a clean key"""
    at = V.plant_indices(n)
    for j, i in enumerate(at):
        words, on, both = V.planted_key(curve, n, [i], start=j + n)
        assert sum(both) == n - 1
        _check_key(ctx, curve, words, on, both, [i], wins=[(0, n), (i, 1), (0, i), (i + 1, n - i - 1)])
    kinds = len(V.non_member_words(curve))
    extra = [i for i in range(1, n - 1) if i not in at][:max(0, kinds - len(at))]
    words, on, both = V.planted_key(curve, n, at + extra)
    assert sum(both) == n - len(at + extra) and (n < 65 or len(at + extra) == kinds)
    _check_key(ctx, curve, words, on, both, at)
    if n > 1:
        words, on, both = V.planted_key(curve, n, [])
        _check_key(ctx, curve, words, on, both, [0, n - 1])


@pytest.mark.parametrize("n", (1, 65, 257))
@pytest.mark.parametrize("curve", V.CURVES)
def test_planted_off_curve_points(ctx, curve, n):
    """records that are not points of the curve (y + 1, limbs at and above p, ..) at the edges, alone and -- on the BLS12 curves -- beside
    non-members: with both bits a record off the curve fails once"""
    at = V.plant_indices(n)
    words, on, both = V.planted_key(curve, n, at, kind="on_curve", start=n)
    assert on == both and sum(on) == n - len(at)
    _check_key(ctx, curve, words, on, both, at)
    if curve in V.BLS12 and n > 1:
        words, on, both = V.planted_key(curve, n, at, kind="both", start=n)
        assert sum(both) < sum(on) < n
        _check_key(ctx, curve, words, on, both, at)


@pytest.mark.parametrize("curve", ("bn254", "pallas"))
def test_cofactor_one_subgroup_is_every_point(ctx, curve):
    """ark-ec's cofactor_is_one(): the subgroup bit alone passes every record, whatever it holds"""
    words, _, _ = V.planted_key(curve, 65, [0, 64], kind="on_curve")
    key = V.upload_words(ctx, curve, words)
    assert V.query(key, 0, 65, False, True) == (0, None, [1] * 65)
    assert key.in_subgroup() is True
    key.free()


def _worker(ladder):
    env = dict(os.environ, PC_HIP_SUBGROUP_LADDER=ladder)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_validate_worker.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "validate worker done, PC_HIP_SUBGROUP_LADDER=" + ladder
    return lines[:-1]


def test_fast_path_and_plain_ladder_agree_through_the_abi():
    """both values of PC_HIP_SUBGROUP_LADDER, a fresh child process each, on keys of 1, 63, 64, 65, 257 and 1000 points with the plants of
    test_planted_non_members, the subgroup bit alone and both bits: the same answers, bit for bit, and the reference's"""
    import _validate_worker as W
    fast, ladder = _worker("0"), _worker("1")
    assert fast == ladder
    want = {}
    for curve in V.BLS12:
        for n in V.SIZES:
            for name, kind, at, start, _ in W.keys(curve, n):
                want[(curve, n, name)] = V.planted_key(curve, n, at, kind=kind, start=start)[2]
    seen, sizes, gated = 0, set(), 0
    for line in fast:
        q = json.loads(line)
        bad, first, flags = V.expect_query(want[(q["curve"], q["n"], q["key"])], q["offset"], q["count"])
        assert (q["bad"], q["first"], q["flags"]) == (bad, first, "".join(map(str, flags))), q
        seen += bad
        sizes.add((q["curve"], q["n"]))
        gated += 1 if q["on_curve"] and bad else 0
    assert sizes == {(c, n) for c in V.BLS12 for n in V.SIZES} and seen > 0 and gated > 0


@pytest.mark.parametrize("curve", V.CURVES)
def test_infinities_and_empty_ranges(ctx, curve):
    n = 65
    key = V.upload_words(ctx, curve, np.zeros((n, V.member_words(curve).shape[1]), dtype=np.uint32))
    for on_curve, subgroup in ((True, True), (True, False), (False, True)):
        assert V.query(key, 0, n, on_curve, subgroup) == (0, None, [1] * n)
        for off in (0, 64, n):
            assert V.query(key, off, 0, on_curve, subgroup) == (0, None, [])
    assert key.in_subgroup() is True
    key.free()


# ---- the cached answer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve", V.CURVES)
def test_generated_keys_are_in_the_subgroup_and_the_answer_carries(ctx, curve):
    """1 after pc_hip_sample_generators (the cofactor was cleared), carried through srs_prefix and ec_fold_from; pc_hip_srs_check agrees"""
    key = ctx.sample_generators(curve, S.IPA_NAME, 0, 64)
    u = np.frombuffer((0x1234567 * (1 << 256) % V.order_r(curve)).to_bytes(32, "little"), dtype=np.uint64).copy()
    assert key.in_subgroup() is True and key.check() == (0, None)
    pre = key.prefix(33)
    assert pre.in_subgroup() is True and pre.check() == (0, None)
    folded = key.fold_from(32, u)
    assert folded.in_subgroup() is True and folded.check() == (0, None)
    folded.free(); pre.free(); key.free()


@pytest.mark.parametrize("curve", V.BLS12)
def test_the_answer_is_asked_again_after_an_upload(ctx, curve):
    """an uploaded key starts unknown: a key with one non-member answers 0, its clean twin 1, a prefix that leaves the non-member out
    1 again (a 0 does not carry), and a fold of the bad key is asked anew"""
    n = 65
    words, _, both = V.planted_key(curve, n, [40])
    bad = V.upload_words(ctx, curve, words)
    good = V.upload_words(ctx, curve, V.member_words(curve)[:n])
    assert bad.in_subgroup() is False and bad.in_subgroup() is False and good.in_subgroup() is True
    assert bad.check(on_curve=False) == (1, 40)
    pre = bad.prefix(40)
    assert pre.in_subgroup() is True
    u = np.frombuffer((7 * (1 << 256) % V.order_r(curve)).to_bytes(32, "little"), dtype=np.uint64).copy()
    folded = bad.fold_from(32, u)            # point 8 of the fold is P_8 + 7 T with T outside the subgroup: the reference decides
    t = S.point_of_words(curve, words[40])
    want = V.in_subgroup(curve, V.add(curve, S.point_of_words(curve, words[8]), S.mul(curve, 7, t)))
    assert folded.in_subgroup() is want and folded.check(on_curve=False) == ((0, None) if want else (1, 8))
    good_fold = good.fold_from(32, u)
    assert good_fold.in_subgroup() is True
    for k in (good_fold, folded, pre, good, bad):
        k.free()


# ---- pc_hip_srs_load_serialized_ex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compressed", (False, True), ids=("uncompressed", "compressed"))
@pytest.mark.parametrize("curve", V.BLS12)
def test_load_with_validation(ctx, curve, compressed):
    import poly_commit_amd as pc
    n, j = 65, 64
    good = V.upload_words(ctx, curve, V.member_words(curve)[:n])
    data = good.serialize(compressed=compressed)
    gt = dict(V.non_member_words(curve))["G + T"]
    one = V.upload_words(ctx, curve, np.array([gt], dtype=np.uint32))
    rec = one.serialize(compressed=compressed)[8:]
    pb = (len(data) - 8) // n
    assert len(rec) == pb
    spoiled = data[:8 + j * pb] + rec + data[8 + (j + 1) * pb:]
    # the clean bytes load under Validate::Yes, and the key knows its answer
    key, used = ctx.load_serialized_srs(curve, data, compressed, validate=True)
    assert used == len(data) and key.n == n and key.in_subgroup() is True
    key.free()
    for what in (pc.CHECK_SUBGROUP, pc.CHECK_SUBGROUP | pc.CHECK_ON_CURVE):
        with pytest.raises(pc.PcHipError) as e:
            ctx.load_serialized_srs(curve, spoiled, compressed, validate=what)
        assert e.value.status == INVALID_ARG and "1 serialized point(s)" in str(e.value) and "index %d" % j in str(e.value)
    # Validate::No in its three spellings loads it; the query then finds exactly that index
    for validate in (None, 0, pc.CHECK_ON_CURVE):
        key, used = ctx.load_serialized_srs(curve, spoiled, compressed, validate=validate)
        assert used == len(spoiled) and key.check() == (1, j) and key.check(subgroup=False) == (0, None)
        assert key.in_subgroup() is False
        key.free()
    with pytest.raises(pc.PcHipError) as e:
        ctx.load_serialized_srs(curve, data, compressed, validate=4)
    assert e.value.status == INVALID_ARG
    one.free(); good.free()


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 64, 65))
def test_g2_check(ctx, n):
    """multiples of the generator, raw twist points (the reference finds them outside the subgroup), records off the twist, infinity"""
    import poly_commit_amd as pc
    kinds, words, on, sub = V.g2_cases()
    members = [i for i, k in enumerate(kinds) if k == "member"]
    special = [kinds.index("raw twist point"), kinds.index("y + 1"), kinds.index("infinity"), kinds.index("coefficient 2 + p"), kinds.index("raw twist point") + 1]
    at = V.plant_indices(n) if n > 1 else []
    rows = [members[i % len(members)] for i in range(n)]
    for j, i in enumerate(at):
        rows[i] = special[j % len(special)]
    if n == 1:
        rows = [special[0]]
    w = np.ascontiguousarray(words[rows])
    want_on = [on[r] for r in rows]
    want_both = [1 if on[r] and sub[r] else 0 for r in rows]
    assert 0 in want_both and (n == 1 or (1 in want_both and 0 in want_on))
    key = pc.G2Srs(ctx, "bls12_381", w.view(np.uint8).reshape(n, 192))
    for off, cnt in V.windows(n, at or [0]):
        assert V.query(key, off, cnt, True, True) == V.expect_query(want_both, off, cnt)
        assert V.query(key, off, cnt, True, False) == V.expect_query(want_on, off, cnt)
    if all(want_on):
        assert V.query(key, 0, n, False, True) == V.expect_query(want_both, 0, n)
    key.free()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------

def test_argument_errors(ctx):
    import poly_commit_amd as pc
    lib = ctx.lib
    key = V.upload_words(ctx, "bn254", V.member_words("bn254")[:8])
    g2 = pc.G2Srs(ctx, "bls12_381", np.zeros((2, 192), dtype=np.uint8))
    other = pc.Context(0)
    bad, first = C.c_size_t(), C.c_size_t()
    for fn, k in ((lib.pc_hip_srs_check, key.h), (lib.pc_hip_g2_srs_check, g2.h)):
        n = 8 if k is key.h else 2
        for args in ((0, n + 1, 3), (n + 1, 0, 3), (1, n, 3), (0, n, 0), (0, n, 4), (0, n, 7)):
            assert fn(ctx.h, k, args[0], args[1], args[2], C.byref(bad), C.byref(first), None) == INVALID_ARG, args
        assert fn(other.h, k, 0, n, 3, C.byref(bad), C.byref(first), None) == INVALID_ARG
        assert fn(ctx.h, None, 0, 0, 3, C.byref(bad), C.byref(first), None) == INVALID_ARG
        assert fn(ctx.h, k, 0, n, 3, None, C.byref(first), None) == INVALID_ARG
        assert fn(ctx.h, k, n, 0, 3, C.byref(bad), None, None) == 0 and bad.value == 0
    out = C.c_int()
    assert lib.pc_hip_srs_in_subgroup(other.h, key.h, C.byref(out)) == INVALID_ARG
    assert lib.pc_hip_srs_in_subgroup(ctx.h, key.h, None) == INVALID_ARG
    other.close(); g2.free(); key.free()
