"""The pure-Python restatement of HyraxPC over ed_on_bls12_381 (tests/harness/te_hyrax.py), the checker of the device path, checked
against itself: its own proofs pass its check, the proved evaluation is the polynomial's, a proof with any one field changed fails,
and an odd or missing number of variables is refused.  No device."""
import numpy as np
import pytest

from harness import te_hyrax as H
from harness import teref as E


def rand_fr(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


def instance(num_vars, seed=0):
    """(key, evals, point, row_coms, state, proof, eval, c) of one commit and open"""
    dim = 1 << (num_vars // 2)
    pp = H.setup(num_vars)
    ck, vk = H.trim(pp)
    assert ck is pp and vk is pp
    evals = rand_fr(100 + num_vars + seed, 1 << num_vars)
    point = rand_fr(200 + num_vars + seed, num_vars)
    rands = rand_fr(300 + num_vars + seed, dim)
    r_eval, r_d, r_b, c = rand_fr(400 + num_vars + seed, 4)
    d = rand_fr(500 + num_vars + seed, dim)
    row_coms, state = H.commit(ck, evals, rands)
    proof, ev = H.open(ck, state, point, r_eval, d, r_d, r_b, c)
    return ck, evals, point, row_coms, state, proof, ev, c


@pytest.mark.parametrize("num_vars", [0, 2, 6])
def test_own_proof_passes_and_proves_the_evaluation(num_vars):
    ck, evals, point, row_coms, state, proof, ev, c = instance(num_vars)
    dim = 1 << (num_vars // 2)
    assert len(ck["com_key"]) == dim and len(row_coms) == dim and len(proof[3]) == dim
    assert all(E.on_curve(p) and E.mul(E.R, p) == E.IDENT for p in ck["com_key"] + [ck["h"]])      # generators of the prime-order subgroup
    assert ev == H.evaluate(evals, point)
    assert H.check(ck, row_coms, point, proof, c)
    # another challenge, another point or another commitment do not verify
    assert not H.check(ck, row_coms, point, proof, (c + 1) % E.R)
    if num_vars:
        other = list(point)
        other[0] = (other[0] + 1) % E.R
        assert not H.check(ck, row_coms, other, proof, c)
        bad = list(row_coms)
        bad[0] = E.add(bad[0], ck["h"])
        assert not H.check(ck, bad, point, proof, c)


@pytest.mark.parametrize("num_vars", [0, 2, 6])
def test_a_proof_with_one_field_changed_fails(num_vars):
    ck, evals, point, row_coms, state, proof, ev, c = instance(num_vars, seed=7)
    g = ck["com_key"][0]
    for k in range(6):
        bad = list(proof)
        if k < 3:
            bad[k] = E.add(bad[k], g)                                  # com_eval, com_d, com_b
        elif k == 3:
            bad[3] = list(bad[3])
            bad[3][-1] = (bad[3][-1] + 1) % E.R                        # one element of z
        else:
            bad[k] = (bad[k] + 1) % E.R                                # z_d, z_b
        assert not H.check(ck, row_coms, point, tuple(bad), c), k
    assert H.check(ck, row_coms, point, proof, c)


def test_a_larger_key_commits_a_smaller_polynomial():
    """com_key[..dim] || h of a larger key: the same commitments as against a key that holds just those generators (the generators of
    a protocol name do not depend on how many are sampled, but h does: it is the LAST one)"""
    big = H.setup(6)
    evals, rands = rand_fr(1, 4), rand_fr(2, 2)
    row_coms, _ = H.commit(big, evals, rands)
    small = dict(com_key=big["com_key"][:2], h=big["h"])
    assert row_coms == H.commit(small, evals, rands)[0]
    assert H.setup(2)["com_key"] == big["com_key"][:2] and H.setup(2)["h"] == big["com_key"][2] != big["h"]


def test_odd_and_missing_num_vars_are_refused():
    for nv in (1, 3, 7, None):
        with pytest.raises(H.InvalidNumberOfVariables):
            H.setup(nv)
    pp = H.setup(2)
    with pytest.raises(H.InvalidNumberOfVariables):
        H.commit(pp, rand_fr(1, 8), rand_fr(2, 2))                      # 3 variables
    with pytest.raises(H.InvalidNumberOfVariables):
        H.commit(pp, rand_fr(1, 16), rand_fr(2, 4))                     # 4 variables on a key of 2 generators (:226)
    ck, evals, point, row_coms, state, proof, ev, c = instance(2)
    with pytest.raises(H.InvalidNumberOfVariables):
        H.open(ck, state, point + [5], 1, [1, 2], 3, 4, c)
    with pytest.raises(H.InvalidNumberOfVariables):
        H.check(ck, row_coms, point + [5], proof, c)
    with pytest.raises(H.IncorrectCommitmentSize):
        H.check(ck, row_coms[:1], point, proof, c)


def test_tensors_are_the_lagrange_weights():
    """l (x) r are the weights of the evaluations: sum_i w_i e_i with w = the tensor of the whole point, rows in the low bits"""
    point = rand_fr(9, 4)
    l, r = H.tensors(point)
    evals = rand_fr(10, 16)
    assert sum(l[i % 4] * r[i // 4] * evals[i] for i in range(16)) % E.R == H.evaluate(evals, point)
