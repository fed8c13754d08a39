"""HyraxPC over ed_on_bls12_381 on the device (poly_commit_amd/te_hyrax.py: pc_hip_te_sample_generators, pc_hip_te_msm_many,
pc_hip_te_fr_lincomb, pc_hip_te_fr_dot, pc_hip_te_msm) against the pure-Python restatement tests/harness/te_hyrax.py, bit for bit: the
key, the row commitments, every field of the proof and the evaluation, at the variable counts of the reference's own tests
(hyrax/tests.rs:106-205: 0, 6, 8, 10) and at 2 and 12; the prefix-plus-h path of a larger key; two polynomials on one key in either
order; and a 20-variable commit on a key with known logarithms."""
import numpy as np
import pytest

from harness import te_hyrax as H
from harness import teref as E

pytestmark = pytest.mark.gpu
CURVE = "ed_on_bls12_381"


def rand_fr(seed, n):
    rnd = np.random.RandomState(seed)
    return [int.from_bytes(rnd.bytes(32), "little") % E.R for _ in range(n)]


def mont(vals):
    return E.scalars_array(list(vals), True)


def ints(arr):
    ri = pow(E.MONT_R, -1, E.R)
    return [int.from_bytes(row.tobytes(), "little") * ri % E.R for row in np.asarray(arr, dtype=np.uint8).reshape(-1, 32)]


def pts(arr):
    return [E.point_from_bytes(row.tobytes()) for row in np.asarray(arr, dtype=np.uint8).reshape(-1, 64)]


def inputs(num_vars, seed=0):
    dim = 1 << (num_vars // 2)
    evals = rand_fr(100 + num_vars + seed, 1 << num_vars)
    point = rand_fr(200 + num_vars + seed, num_vars)
    rands = rand_fr(300 + num_vars + seed, dim)
    r_eval, r_d, r_b, c = rand_fr(400 + num_vars + seed, 4)
    d = rand_fr(500 + num_vars + seed, dim)
    return evals, point, rands, r_eval, d, r_d, r_b, c


def dev_commit(T, key, evals, rands):
    import torch
    return T.commit(key, torch.from_numpy(mont(evals)).cuda(), mont(rands))


def dev_open(T, key, state, point, r_eval, d, r_d, r_b, c):
    return T.open(key, state, mont(point), mont([r_eval])[0], mont(d), mont([r_d])[0], mont([r_b])[0], mont([c])[0])


def proof_as_ints(proof):
    com_eval, com_d, com_b, z, z_d, z_b = proof
    return (pts(com_eval)[0], pts(com_d)[0], pts(com_b)[0], ints(z), ints(z_d)[0], ints(z_b)[0])


@pytest.mark.parametrize("num_vars", [0, 2, 6, 8, 10, 12])
def test_te_hyrax_against_the_restatement(ctx, num_vars):
    from poly_commit_amd import te_hyrax as T
    dim = 1 << (num_vars // 2)
    evals, point, rands, r_eval, d, r_d, r_b, c = inputs(num_vars)
    ref_key = H.setup(num_vars)
    want_coms, want_state = H.commit(ref_key, evals, rands)
    want_proof, want_ev = H.open(ref_key, want_state, point, r_eval, d, r_d, r_b, c)
    assert want_ev == H.evaluate(evals, point) and H.check(ref_key, want_coms, point, want_proof, c)
    key = T.setup(ctx, num_vars)
    try:
        ck, vk = T.trim(key)
        assert ck is key and vk is key
        assert pts(key.com_key()) == ref_key["com_key"] and pts(key.h) == [ref_key["h"]] and pts(key.g0) == ref_key["com_key"][:1]
        assert len(key.full) == dim + 1
        row_coms, state = dev_commit(T, ck, evals, rands)
        assert pts(row_coms) == want_coms
        proof, ev = dev_open(T, ck, state, point, r_eval, d, r_d, r_b, c)
        assert ints(ev) == [want_ev]
        assert proof_as_ints(proof) == want_proof
        cm = mont([c])[0]
        pm = mont(point)
        assert T.check(vk, row_coms, pm, proof, cm)
        assert H.check(ref_key, pts(row_coms), point, proof_as_ints(proof), c)
        # one field changed: both checks fail
        g = key.g0
        from poly_commit_amd import _ffi
        for k in range(6):
            bad = list(proof)
            if k < 3:
                bad[k] = _ffi.te_points_sum(CURVE, np.stack([bad[k], g]))
            elif k == 3:
                zi = ints(bad[3])
                zi[-1] = (zi[-1] + 1) % E.R
                bad[3] = mont(zi)
            else:
                bad[k] = mont([(ints(bad[k])[0] + 1) % E.R])[0]
            assert not T.check(vk, row_coms, pm, tuple(bad), cm), k
            assert not H.check(ref_key, pts(row_coms), point, proof_as_ints(tuple(bad)), c), k
        assert not T.check(vk, row_coms, pm, proof, mont([c + 1])[0])
    finally:
        key.close()


def test_te_hyrax_refuses_odd_and_missing_num_vars(ctx):
    from poly_commit_amd import te_hyrax as T
    import torch
    for nv in (1, 5, None):
        with pytest.raises(T.InvalidNumberOfVariables):
            T.setup(ctx, nv)
    key = T.setup(ctx, 2)
    try:
        with pytest.raises(T.InvalidNumberOfVariables):
            T.commit(key, torch.zeros((8, 32), dtype=torch.uint8).cuda(), mont([1, 2]))          # 3 variables
        with pytest.raises(T.InvalidNumberOfVariables):
            T.commit(key, torch.zeros((16, 32), dtype=torch.uint8).cuda(), mont([1, 2, 3, 4]))   # 4 variables on a key of 2 generators
    finally:
        key.close()


def test_te_hyrax_larger_key_smaller_polynomial(ctx):
    """A key made for 10 variables used for a polynomial of 6: the extended key com_key[..8] || h is made once and kept; the same bits
    as the restatement over those generators, and the proof verifies on the device."""
    from poly_commit_amd import te_hyrax as T
    evals, point, rands, r_eval, d, r_d, r_b, c = inputs(6, seed=3)
    ref_key = H.setup(10)
    want_coms, want_state = H.commit(ref_key, evals, rands)
    want_proof, want_ev = H.open(ref_key, want_state, point, r_eval, d, r_d, r_b, c)
    assert H.check(ref_key, want_coms, point, want_proof, c)
    key = T.setup(ctx, 10)
    try:
        row_coms, state = dev_commit(T, key, evals, rands)
        ext = key.ext(8)
        assert ext is not key.full and len(ext) == 9 and key.ext(8) is ext
        assert pts(ext.read(0, 9)) == ref_key["com_key"][:8] + [ref_key["h"]]
        assert pts(row_coms) == want_coms
        proof, ev = dev_open(T, key, state, point, r_eval, d, r_d, r_b, c)
        assert ints(ev) == [want_ev] and proof_as_ints(proof) == want_proof
        assert T.check(key, row_coms, mont(point), proof, mont([c])[0])
        # the full dimension on the same key afterwards
        e10 = inputs(10, seed=4)
        coms10, _ = dev_commit(T, key, e10[0], e10[2])
        assert pts(coms10)[:2] == H.commit(ref_key, e10[0], e10[2])[0][:2]
    finally:
        key.close()


def test_te_hyrax_two_polynomials_in_either_order(ctx):
    """Two polynomials committed and opened one after the other on one key: nothing of one call is left in the next (the cached table,
    the pipelines, the staging buffers)."""
    from poly_commit_amd import te_hyrax as T
    a, b = inputs(6, seed=11), inputs(6, seed=12)
    key = T.setup(ctx, 6)
    try:
        def run(order):
            out = {}
            states = {}
            for name, x in order:
                out[name] = [dev_commit(T, key, x[0], x[2])]
                states[name] = out[name][0][1]
            for name, x in order:
                out[name].append(dev_open(T, key, states[name], x[1], *x[3:]))
            return {name: (v[0][0].tobytes(), [np.asarray(f).tobytes() for f in v[1][0]], v[1][1].tobytes()) for name, v in out.items()}
        first = run([("a", a), ("b", b)])
        second = run([("b", b), ("a", a)])
        assert first == second
        ref_key = H.setup(6)
        for name, x in (("a", a), ("b", b)):
            coms, st = H.commit(ref_key, x[0], x[2])
            assert first[name][0] == E.points_array(coms).tobytes()
            assert ints(np.frombuffer(first[name][2], dtype=np.uint8)) == [H.open(ref_key, st, x[1], *x[3:])[1]]
    finally:
        key.close()


def test_te_hyrax_commit_20_variables_on_a_known_key(ctx):
    """num_vars = 20, commit only: 1024 rows of 1025 pairs in one pass, on a key of known multiples of G.  16 sampled rows against
    (sum_c row[c] k_c + r k_h) G, and the sum of all rows by linearity."""
    import torch
    from poly_commit_amd import _ffi
    from poly_commit_amd import te_hyrax as T
    nv, dim = 20, 1024
    kk = [(i * 0x9e3779b97f4a7c15 + 0x5eed) ** 3 % E.R for i in range(dim + 1)]
    fb = E.fixed_base(E.GEN)
    key = T.TeHyraxKey(ctx, ctx.upload_te_srs(CURVE, E.points_array(fb.mul_many(kk))), nv)
    try:
        rnd = np.random.RandomState(20)
        raw = np.frombuffer(rnd.bytes(32 << nv), dtype=np.uint8).reshape(1 << nv, 32).copy()
        raw[:, 31] &= 0x07                                    # every 32 bytes a residue below 2^251 < r: taken as the Montgomery form of v = raw / 2^256
        rands = rand_fr(21, dim)
        row_coms, _ = T.commit(key, torch.from_numpy(raw).cuda(), mont(rands))
        ri = pow(E.MONT_R, -1, E.R)
        words = raw.view(np.uint32).reshape(dim, dim, 8)       # [column c][row i]: evals[c * dim + i]

        def as_int(w):
            return sum(int(x) << (32 * k) for k, x in enumerate(w))
        rows = list(range(0, dim, 73)) + [dim - 1]
        rows = rows[:15] + [dim - 1]
        logs = [(sum(as_int(words[c, i]) * kk[c] for c in range(dim)) * ri + rands[i] * kk[dim]) % E.R for i in rows]
        assert [E.point_from_bytes(row_coms[i].tobytes()) for i in rows] == fb.mul_many(logs)
        col = words.astype(np.uint64).sum(axis=1)              # per column, the sum over the rows, word by word (below 2^42)
        total = (sum(as_int(col[c]) * kk[c] for c in range(dim)) * ri + sum(rands) * kk[dim]) % E.R
        assert E.point_from_bytes(_ffi.te_points_sum(CURVE, row_coms).tobytes()) == fb.mul_many([total])[0]
    finally:
        key.close()
