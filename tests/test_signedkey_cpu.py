"""tests/harness/signedkey.py on the CPU: the keys are what their logarithms say, and the oracle's two MSMs (bucket method and naive)
return the integer-exact expectation on every cancelling layout, on all four curves.  The device tests (tests/test_msm_cancel_gpu.py)
then compare against the integer expectation, with the oracle's bucket method as a second opinion."""
import numpy as np
import pytest

import oracle_lib as O
from harness import signedkey as SK


@pytest.mark.parametrize("curve", SK.CURVES)
def test_pool_and_keys_are_what_their_logarithms_say(curve):
    ref, r = O.ref(curve), SK.modulus(curve)
    ks, words = SK.pool(curve)
    assert len(set(ks)) == 8 and all(k % 2 == 1 and 0 < k < r for k in ks)
    assert len({k for k in ks} | {r - k for k in ks}) == 16                      # Q_i != +-Q_j
    G = ref.generator(curve)
    key = SK.signed(curve, 130, holes=True)
    pts = O.array_to_points(curve, key.bases)
    for j in (0, 1, 2, 3, 10, 11, 12, 17, 75, 128, 129):
        e = key.logs[j]
        assert pts[j] == (ref.ec_mul(curve, e % r, G) if e else None), j
        assert (e == 0) == (j % 64 == 11) == bool(key.is_hole(j))
        if j % 2 == 0 and not key.is_hole(j + 1):
            assert key.logs[j + 1] == -e and pts[j + 1] == ref.ec_neg(curve, pts[j])
    assert SK.unsigned(curve, 20).logs == [ks[(j // 2) % 8] for j in range(20)]
    assert SK.one_base(curve, 5).logs == [ks[0]] * 5
    h = SK.halves(curve, 40)
    assert h.logs[:20] == [ks[j % 8] for j in range(20)] and h.logs[20:] == [-e for e in h.logs[:20]]
    assert (h.bases[:20, :h.bases.shape[1] // 2] == h.bases[20:, :h.bases.shape[1] // 2]).all()      # the same x


def _cases(curve, n, start=0):
    """(name, key, scalars, sums to infinity) of every layout on the key it is meant for"""
    sg = SK.signed(curve, n + start, holes=True)
    lay = SK.layouts(curve, n, 0x1A70 + n, start, holes=True)
    out = [(name, sg, lay[name], name != "all_but_one") for name in ("const", "pairwise", "pairwise_few", "all_but_one")]
    out.append(("opposite_scalars", SK.unsigned(curve, n + start), SK.layouts(curve, n, 0x1A71 + n, start)["opposite_scalars"], True))
    out.append(("const on one_base", SK.one_base(curve, n + start), SK.const(curve, n, 0x1A72 + n), False))
    out.append(("all_but_one on const", sg, SK.all_but_one_on_const(curve, n, 0x1A73 + n, start, holes=True), False))
    return out


@pytest.mark.parametrize("n", [64, 700])
@pytest.mark.parametrize("curve", SK.CURVES)
def test_oracle_msms_return_the_integer_expectation(curve, n):
    for start in (0, 7):
        for name, key, s, inf in _cases(curve, n, start):
            want = SK.expected(key, s, start)
            assert (not want.any()) == inf, (name, start)
            sc = SK.limbs(s)
            b = np.ascontiguousarray(key.bases[start:])
            assert (O.msm_pippenger(curve, b, sc, 4, 1) == want).all(), (name, start, "pippenger")
            assert (O.msm_naive(curve, b, sc) == want).all(), (name, start, "naive")


def test_layouts_shapes():
    """what the layouts promise: equal scalars on the two members of a pair, zero where the partner is missing, one changed entry"""
    curve, n = "bn254", 700
    for start in (0, 5, 7):
        lay = SK.layouts(curve, n, 3, start, holes=True)
        c, p, ab = lay["const"], lay["pairwise"], lay["all_but_one"]
        assert len({v for v in c if v}) == 1 and sum(1 for v in c if not v) <= 2 + n // 64 + 1
        lone = [i for i in range(n) if not (start <= ((start + i) ^ 1) < start + n) or ((start + i) ^ 1) % 64 == 11]
        assert [i for i in range(n) if not c[i]] == lone == [i for i in range(n) if not p[i]]
        for i in range(n - 1):
            if (start + i) % 2 == 0 and i not in lone:
                assert p[i] == p[i + 1] and c[i] == c[i + 1]
        assert sum(1 for a, b in zip(p, ab) if a != b) == 1
        assert len({v for v in lay["pairwise_few"] if v}) <= 5
