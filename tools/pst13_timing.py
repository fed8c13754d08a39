"""Time MarlinPST13's commit and open on the device (BLS12-381).

Per shape (num_vars, degree) in {(10, 10), (8, 16)} (or the pairs given as n,d arguments): a TRUE key of M = C(n + d, n) points made
by the setup path (pc_hip_pst13_monomial_evals, pc_hip_fixed_base_batch_mul) with its window table, and two resident polynomials:
dense random coefficients, and the reference's own sparse shape (a sum of univariates, n d + 1 terms).
  - pc_hip_pst13_commit against one blocking pc_hip_msm of the same M scalars (they are the same call for a dense vector: the
    difference is noise; from terms it adds the scatter).
  - pc_hip_pst13_open against what a caller could do today with the quotient vectors in hand: n blocking pc_hip_msm calls of M pairs
    each on the SAME quotients, zero-extended to the key's length (no prefix argument).  That baseline contains no division;
    pc_hip_pst13_divide alone is timed beside it.  The sides alternate in one process: warm-up, then median / min / max.
Timing needs a GPU: there is no fallback.  Prints one JSON line per measurement."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import oracle_lib as O  # noqa: E402
import poly_commit_amd as pc  # noqa: E402
from poly_commit_amd import _ffi  # noqa: E402

CURVE = "bls12_381"
REPS = int(os.environ.get("PC_PST13_REPS", "7"))


def alternate(fns, warm=2, reps=REPS):
    """{name: (median, min, max)} in ms of blocking calls, the sides taking turns"""
    for _ in range(warm):
        for f in fns.values():
            f()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)) for k, v in out.items()}


def run(ctx, n, d):
    M = _ffi.pst13_key_len(n, d)
    prefix = [_ffi.pst13_key_len(n - i, d) if i < n else 1 for i in range(n)]
    rnd = O.f_to_mont(CURVE, 1, O.gen_scalars(CURVE, 0x9513 + 100 * n + d, 2 * n + 2 + n * d + 1))
    betas, z, seed, uni_coeffs = rnd[:n], rnd[n:2 * n], rnd[2 * n], rnd[2 * n + 1:]
    ev = torch.empty((M, 4), dtype=torch.int64, device="cuda")
    ctx.pst13_monomial_evals(CURVE, n, d, betas, ev.data_ptr())
    key_pts = torch.empty((M, 12), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(CURVE, O.gen_bases(CURVE, 1)[0], ev.data_ptr(), M, key_pts.data_ptr())
    srs = ctx.upload_srs(CURVE, key_pts.data_ptr(), n=M)
    del key_pts
    srs.precompute()
    # dense: the powers of an element -- uniform-looking scalars; sparse: the constant and X_j^t, t = 1 .. d, for every variable
    dense = ev
    ctx.fr_powers(CURVE, seed, M, dense.data_ptr())
    exps = np.zeros((n * d + 1, n), dtype=np.uint8)
    for j in range(n):
        for t in range(1, d + 1):
            exps[1 + j * d + t - 1, j] = t
    sparse = torch.zeros((M, 4), dtype=torch.int64, device="cuda")
    ctx.pst13_scatter(CURVE, n, d, exps, uni_coeffs, sparse.data_ptr())
    total = sum(prefix)
    quot = torch.empty((total, 4), dtype=torch.int64, device="cuda")
    ext = torch.zeros((n, M, 4), dtype=torch.int64, device="cuda")      # the quotients zero-extended to M pairs
    for name, poly in (("dense", dense), ("sparse", sparse)):
        res = alternate({"pst13_commit": lambda: srs.pst13_commit(n, d, dense=poly.data_ptr()), "msm": lambda: srs.msm(poly.data_ptr(), n=M, montgomery=True)})
        line = {"what": "commit", "shape": [n, d], "M": M, "polynomial": name, "pst13_commit_ms": res["pst13_commit"], "msm_ms": res["msm"]}
        if name == "sparse":
            line["pst13_commit_from_terms_ms"] = alternate({"t": lambda: srs.pst13_commit(n, d, exps=exps, coeffs=uni_coeffs)})["t"]
            line["terms"] = int(exps.shape[0])
        print(json.dumps(line), flush=True)
        offs, _ = ctx.pst13_divide(CURVE, n, d, poly.data_ptr(), z, quot.data_ptr(), total)
        ext.zero_()
        for i in range(n):
            ext[i, :prefix[i]] = quot[offs[i]:offs[i] + prefix[i]]
        per_msm = [[] for _ in range(n)]

        def baseline():
            for i in range(n):
                t0 = time.perf_counter()
                srs.msm(ext[i].data_ptr(), n=M, montgomery=True)
                per_msm[i].append((time.perf_counter() - t0) * 1e3)

        res = alternate({"pst13_open": lambda: srs.pst13_open(n, d, z, dense=poly.data_ptr()), "n_msms_of_M": baseline,
                         "pst13_divide": lambda: ctx.pst13_divide(CURVE, n, d, poly.data_ptr(), z, quot.data_ptr(), total)})
        got = srs.pst13_open(n, d, z, dense=poly.data_ptr())[0]
        assert all((got[i] == srs.msm(ext[i].data_ptr(), n=M, montgomery=True)[0]).all() for i in range(n)), "the baseline's scalars are not the call's"
        new, base = res["pst13_open"], res["n_msms_of_M"]
        print(json.dumps({"what": "open", "shape": [n, d], "M": M, "polynomial": name, "pst13_open_ms": new, "n_msms_of_M_ms": base,
                          "pst13_divide_ms": res["pst13_divide"], "baseline_over_open": round(base[0] / new[0], 2),
                          "pairs_open": total, "pairs_baseline": n * M, "msm_pairs": ctx.last_pst13_shape()[1],
                          "per_msm_of_M_ms": [round(statistics.median(v[2:]), 3) for v in per_msm]}), flush=True)
    srs.free()


def main():
    shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[1:]] or [(10, 10), (8, 16)]
    ctx = pc.Context(0)
    for n, d in shapes:
        run(ctx, n, d)
    ctx.close()


if __name__ == "__main__":
    main()
