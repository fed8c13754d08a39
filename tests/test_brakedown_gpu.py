"""GPU parity of the Brakedown code through the C ABI (pc_hip_brakedown_*) against the Python restatement in
tests/harness/brakedown.py: encode, commit (encoded matrix, leaves, nodes, root), commit / open / check of MultilinearBrakedown,
the reference's benchmark size, rejection of malformed codes on a live context, residency.  All comparisons are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyref as R
from harness import brakedown as B
from harness.brakedown import FIELD_ID, driver, flat_arrays, malformed, messages

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254", "pallas"]


def dev_encode_host(code, dev_code, msgs):
    flat = B.monts(code.curve, [x for row in msgs for x in row]).reshape(len(msgs), code.m, 4)
    out = dev_code.encode(np.ascontiguousarray(flat))
    return [B.ints(code.curve, out[r]) for r in range(len(msgs))], out


def dev_encode_device(code, dev_code, msgs):
    import torch
    flat = B.monts(code.curve, [x for row in msgs for x in row]).reshape(len(msgs), code.m, 4)
    x = torch.from_numpy(np.ascontiguousarray(flat).view(np.int64)).cuda()
    y = torch.full((len(msgs), code.m_ext, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()      # torch's fill is only queued and the library's streams do not wait for torch's: finish it before the library writes
    dev_code.encode(x, rows=len(msgs), out=y)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint64)


def check_encode(ctx, code, row_counts, seed):
    dev_code = code.upload(ctx)
    try:
        assert dev_code.codeword_len == code.m_ext
        for rows in row_counts:
            msgs = messages(code, rows, seed + rows)
            want = [B.encode(code, m) for m in msgs]
            got, raw = dev_encode_host(code, dev_code, msgs)
            assert got == want, (code.curve, code.m, rows, "host -> host")
            assert all(int.from_bytes(raw[r, j].tobytes(), "little") < code.p for r in range(rows) for j in range(0, code.m_ext, 37)), "canonical residues"
            assert (dev_encode_device(code, dev_code, msgs) == raw).all(), (code.curve, code.m, rows, "device -> device")
    finally:
        dev_code.free()


# ---- 1. encode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("nv", [10, 12, 16])
def test_encode_default_codes(ctx, curve, nv):
    n, code = B.default_code(curve, nv, 0x1000 + nv)
    check_encode(ctx, code, sorted({1, 2, n}), 0x77)


@pytest.mark.parametrize("curve", CURVES)
def test_encode_ragged_and_base_codes(ctx, curve):
    check_encode(ctx, B.ragged_code(curve), (1, 2, 3, 65), 0x88)
    check_encode(ctx, B.base_code(curve, 17), (1, 2, 64), 0x99)


# ---- 2. commit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_hash,tree_hash,len_prefix", [("blake2s", "sha256", True), ("sha256", "blake2s", False), ("blake2s", "blake2s", False), ("sha256", "sha256", True)])
def test_commit_equals_restatement_and_the_three_steps(ctx, col_hash, tree_hash, len_prefix):
    curve, nv = "bn254", 12
    n, code = B.default_code(curve, nv, 0x2000)
    evals = messages(B.base_code(curve, 1 << nv), 1, 0x21)[0]
    want = B.ref_commit(code, n, evals, col_hash, tree_hash, len_prefix)
    dev_code = code.upload(ctx)
    try:
        mat = B.monts(curve, evals).reshape(n, code.m, 4)
        ext = np.zeros((n, code.m_ext, 4), dtype=np.uint64)
        nodes, leaves = dev_code.commit(np.ascontiguousarray(mat), col_hash=col_hash, tree_hash=tree_hash, len_prefix=len_prefix, ext_out=ext)
        assert [B.ints(curve, ext[r]) for r in range(n)] == want["ext"]
        assert [bytes(x) for x in leaves] == want["leaves"]
        assert [bytes(x) for x in nodes] == want["nodes"] and bytes(nodes[0]) == want["root"]
        # the composition of the single steps
        ext2 = dev_code.encode(np.ascontiguousarray(mat))
        leaves2 = ctx.column_hash(curve, ext2, col_hash)
        nodes2 = ctx.merkle_tree(leaves2, tree_hash, len_prefix)
        assert (ext2 == ext).all() and (leaves2 == leaves).all() and (nodes2 == nodes).all()
    finally:
        dev_code.free()


# ---- 3. commit, open, check ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,nv", [("bn254", 12), ("bls12_381", 16)])
def test_multilinear_brakedown_commit_open_check(ctx, curve, nv):
    import torch
    fr = R.CURVES[curve]["fr"]
    p = B.field_p(curve)
    n, code = B.default_code(curve, nv, 0x3000 + nv)
    evals = R.gen_scalars(fr, 0x31, 1 << nv)
    point = R.gen_scalars(fr, 0x32, nv)
    want = B.ref_commit(code, n, evals)
    dev_code = code.upload(ctx)
    try:
        com, state = B.commit(ctx, code, dev_code, n, torch.from_numpy(B.monts(curve, evals).view(np.int64)).cuda())
        assert (com["n_rows"], com["n_cols"], com["n_ext_cols"], com["root"]) == (n, code.m, code.m_ext, want["root"])
        t = B.num_queries(curve, code.m_ext)
        assert t == R.calculate_t(p.bit_length(), 128, (61 * 1000, 1521 * 1000), code.m_ext) and 0 < t <= code.m_ext
        idx = [(i * 7919 + 13) % code.m_ext for i in range(t)]
        idx[0], idx[1] = code.m_ext - 1, code.m_ext - 2            # the last leaves: the one beside the tree's padding included
        ab = B.tensor(curve, point, code.m)
        r = R.gen_scalars(fr, 0x33, n)
        pr = B.open(ctx, code, state, idx, B.monts(curve, r), ab)
        want_pr = B.ref_open(code, want, idx, r, ab)
        assert B.ints(curve, pr["v"]) == want_pr["v"] and B.ints(curve, pr["well_formedness"]) == want_pr["well_formedness"]
        assert [B.ints(curve, c) for c in pr["columns"]] == want_pr["columns"] and pr["paths"] == want_pr["paths"]
        value = R.mle_evaluate(fr, evals, point)
        assert sum(x * y for x, y in zip(want_pr["v"], ab[0])) % p == value          # <v, a> is the multilinear extension's value
        args = (ctx, code, dev_code, com)
        rm = B.monts(curve, r)
        assert B.check(*args, B.monts(curve, [value])[0], pr, idx, rm, ab) is True
        assert B.ref_check(code, want, value, want_pr, idx, r, ab) is True
        assert B.check(*args, B.monts(curve, [value + 1])[0], pr, idx, rm, ab) is False
        bad = dict(pr); bad["columns"] = pr["columns"].copy(); bad["columns"][1, 0, 0] ^= np.uint64(1)
        with pytest.raises(B.InvalidCommitment):
            B.check(*args, B.monts(curve, [value])[0], bad, idx, rm, ab)
        bad = dict(pr); bad["paths"] = list(pr["paths"])
        i0, sib, path = bad["paths"][2]
        bad["paths"][2] = (i0, sib, [bytes([path[0][0] ^ 1]) + path[0][1:]] + list(path[1:]))
        with pytest.raises(B.InvalidCommitment):
            B.check(*args, B.monts(curve, [value])[0], bad, idx, rm, ab)
        bad = dict(pr); bad["well_formedness"] = pr["well_formedness"].copy(); bad["well_formedness"][0, 0] ^= np.uint64(1)
        with pytest.raises(B.InvalidCommitment):
            B.check(*args, B.monts(curve, [value])[0], bad, idx, rm, ab)
    finally:
        dev_code.free()


@pytest.mark.parametrize("curve,nv", [("bn254", 12), ("pallas", 16)])
def test_cpp_mirror_device_encode(curve, nv):
    """poly_commit_amd/host/brakedown.hpp: the code made by make_mat, uploaded and encoded through the ABI equals the mirror's host
    encode (which the CPU suite pins to the restatement)."""
    r = subprocess.run([driver(), "device", str(FIELD_ID[curve]), str(nv), str(0x3C00 + nv)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "device encode OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("curve,nv", [("bn254", 12), ("bls12_381", 16)])
def test_cpp_mirror_commit_open_check(curve, nv, tmp_path):
    """BrakedownPCS of host/brakedown.hpp: the driver commits, opens and checks (honest proof accepted, a wrong value refused, an
    altered column, path node and well-formedness vector each InvalidCommitment; at num_vars 16 the first queried column is the one
    beside the tree's padding); its root, v and well-formedness vector equal the restatement's."""
    seed = 0x3D00 + nv
    out = tmp_path / "pcs.bin"
    r = subprocess.run([driver(), "pcs", str(FIELD_ID[curve]), str(nv), str(seed), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "commit/open/check OK" in r.stdout, r.stdout + r.stderr
    n, code = B.default_code(curve, nv, seed)
    ge, gp, gr = B.Gen(seed + 1), B.Gen(seed + 2), B.Gen(seed + 3)
    evals = [ge.nonzero(code.p) for _ in range(1 << nv)]
    point = [gp.nonzero(code.p) for _ in range(nv)]
    rr = [gr.nonzero(code.p) for _ in range(n)]
    want = B.ref_commit(code, n, evals)
    t = B.num_queries(curve, code.m_ext)
    assert "t = %d)" % t in r.stdout
    idx = [code.m_ext - 1] + [(i * 7919 + 13) % code.m_ext for i in range(1, t)]
    ab = B.tensor(curve, point, code.m)
    pr = B.ref_open(code, want, idx, rr, ab)
    raw = out.read_bytes()
    assert len(raw) == 32 + 64 * code.m and raw[:32] == want["root"]
    got = B.ints(curve, np.frombuffer(raw[32:], dtype="<u8").reshape(-1, 4))
    assert got[:code.m] == pr["v"] and got[code.m:] == pr["well_formedness"]
    assert B.ref_check(code, want, R.mle_evaluate(R.CURVES[curve]["fr"], evals, point), pr, idx, rr, ab) is True


# ---- 4. the reference's benchmark size -------------------------------------------------------------------------------------------------------
def test_commit_at_the_reference_benchmark_size(ctx):
    """brakedown_ml_times.rs, BN254, num_vars = 20: 32 x 32768 -> 32 x 49841."""
    curve, nv = "bn254", 20
    n, code = B.default_code(curve, nv, 0x4000)
    assert (n, code.m, code.m_ext) == (32, 32768, 49841)
    evals = R.gen_scalars(R.CURVES[curve]["fr"], 0x41, 1 << nv)
    want = B.ref_commit(code, n, evals)
    dev_code = code.upload(ctx)
    try:
        mat = np.ascontiguousarray(B.monts(curve, evals).reshape(n, code.m, 4))
        ext = np.zeros((n, code.m_ext, 4), dtype=np.uint64)
        nodes, leaves = dev_code.commit(mat, ext_out=ext)
        assert bytes(nodes[0]) == want["root"] and [bytes(x) for x in leaves] == want["leaves"]
        assert B.ints(curve, ext.reshape(-1, 4)) == [x for row in want["ext"] for x in row]
    finally:
        dev_code.free()


# ---- 5. malformed arrays on a live context ----------------------------------------------------------------------------------------------------
def test_malformed_codes_are_rejected_before_the_device(ctx):
    curve = "bn254"
    _, code = B.default_code(curve, 10, 0x5000)
    _, _, _, val = flat_arrays(code)
    before = ctx.bytes_resident()["device_total"]
    for name, dm, ip, ci, m_ext in malformed(code):
        h = C.c_void_p()
        rc = ctx.lib.pc_hip_brakedown_code_create(ctx.h, 1, code.m, m_ext, len(dm) // 6, dm.ctypes.data, ip.ctypes.data, ci.ctypes.data, val.ctypes.data, len(ci), C.byref(h))
        assert rc == -1 and not h.value, name
        assert ctx.bytes_resident()["device_total"] == before, name
    check_encode(ctx, code, (2,), 0x51)


# ---- 6. residency ----------------------------------------------------------------------------------------------------------------------------
def test_two_codes_alive_free_trim_and_bytes_resident(ctx):
    _, ca = B.default_code("bn254", 12, 0x6000)
    _, cb = B.default_code("pallas", 10, 0x6001)
    ma, mb = messages(ca, 2, 1), messages(cb, 3, 2)
    wa, wb = [B.encode(ca, m) for m in ma], [B.encode(cb, m) for m in mb]
    before = ctx.bytes_resident()["device_total"]
    da = ca.upload(ctx)
    after_a = ctx.bytes_resident()["device_total"]
    assert after_a - before >= ca.nnz * 36 + 4 * sum(mt.m + 1 for mt in ca.a_mats + ca.b_mats)      # col_ind, val and ind_ptr of every matrix
    db = cb.upload(ctx)
    assert ctx.bytes_resident()["device_total"] - after_a >= cb.nnz * 36
    for _ in range(2):
        assert dev_encode_host(ca, da, ma)[0] == wa
        assert dev_encode_host(cb, db, mb)[0] == wb
    da.free()
    assert dev_encode_host(cb, db, mb)[0] == wb
    ctx.trim()
    assert dev_encode_host(cb, db, mb)[0] == wb
    ctx.trim()
    with_b = ctx.bytes_resident()["device_total"]
    db.free()
    assert with_b - ctx.bytes_resident()["device_total"] >= cb.nnz * 36
    # a code that is never freed is released with its context
    import poly_commit_amd as pc
    own = pc.Context(0)
    leaked = cb.upload(own)
    assert own.bytes_resident()["device_total"] > 0
    own.close()
    leaked.free()                                                   # the tombstone: deletes the host object only
