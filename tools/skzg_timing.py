"""Time streaming_kzg's commit_folding and open_folding on the device (BLS12-381, k = 3 points, depth = log2 n).

Per log2 n in {20, 24} (or the sizes given): a TRUE key of n powers of a random tau with its window table, a resident polynomial.
  - pc_hip_kzg_commit_folding against the composition a caller could write before it existed: the SAME levels, already folded and
    resident, committed by one blocking pc_hip_msm each.  That baseline contains no folding.  The two sides alternate in one process:
    warm-up, then the median / min / max of the repeats; the per-level times of the baseline are the timeline.
  - pc_hip_kzg_open_folding, and its final MSM alone: the same L_1 - k scalars (made here from pc_hip_fold_tree, pc_hip_poly_div_multi
    per level and pc_hip_fr_lincomb) through pc_hip_msm.  The difference is the price of the folds, divisions and the combination;
    the launches of those are pc_hip_last_skzg_launches.
Timing needs a GPU: there is no fallback.  Prints one JSON line per measurement."""
import ctypes as C
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

CURVE = "bls12_381"
K = 3
REPS = int(os.environ.get("PC_SKZG_REPS", "7"))


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


def run(ctx, log_n):
    n = 1 << log_n
    depth = log_n
    rnd = O.f_to_mont(CURVE, 1, O.gen_scalars(CURVE, 0x5C26 + log_n, 4 + 2 * depth + K))
    tau, rhos, etas, pts = rnd[0], rnd[4:4 + depth], rnd[4 + depth:4 + 2 * depth], rnd[4 + 2 * depth:]
    pw = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    ctx.fr_powers(CURVE, tau, n, pw.data_ptr())
    key_pts = torch.empty((n, 12), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(CURVE, O.gen_bases(CURVE, 1)[0], pw.data_ptr(), n, key_pts.data_ptr())
    srs = ctx.upload_srs(CURVE, key_pts.data_ptr(), n=n)
    del key_pts
    srs.precompute()
    # the polynomial: the powers of another element -- uniform-looking scalars without a 2^24-element host array
    ctx.fr_powers(CURVE, rnd[1], n, pw.data_ptr())
    poly = pw
    lens = [(n + (1 << i) - 1) >> i for i in range(1, depth + 1)]
    tree = torch.empty((sum(lens), 4), dtype=torch.int64, device="cuda")
    offs = ctx.fold_tree(CURVE, poly.data_ptr(), rhos, tree.data_ptr(), sum(lens), n=n)
    level_ptr = [tree.data_ptr() + 32 * o for o in offs]

    # ---- commit_folding against one blocking MSM per resident level
    per_level = [[] for _ in lens]

    def baseline():
        for i, (p, ln) in enumerate(zip(level_ptr, lens)):
            t0 = time.perf_counter()
            srs.msm(p, n=ln, montgomery=True)
            per_level[i].append((time.perf_counter() - t0) * 1e3)

    res = alternate({"commit_folding": lambda: srs.kzg_commit_folding(poly.data_ptr(), rhos, n=n), "msm_per_level": baseline})
    new, base = res["commit_folding"], res["msm_per_level"]
    print(json.dumps({"what": "commit_folding", "log_n": log_n, "depth": depth, "commit_folding_ms": new, "msm_per_level_ms": base,
                      "baseline_spread_ms": round(base[2] - base[1], 3), "new_minus_baseline_ms": round(new[0] - base[0], 3),
                      "per_level_msm_ms": [round(statistics.median(v[2:]), 3) for v in per_level], "level_lens": lens,
                      "fold_launches": ctx.last_skzg_launches()[0], "small_level_crossover": "not measured (the many-MSM pass is not built)"}), flush=True)

    # ---- open_folding against its final MSM alone: the same scalars, made step by step
    m = lens[0] - K
    quot = torch.zeros((sum(max(ln - K, 0) for ln in lens), 4), dtype=torch.int64, device="cuda")
    rem = np.zeros((K, 4), dtype=np.uint64)
    qptr, at = [], quot.data_ptr()
    for p, ln in zip(level_ptr, lens):
        qptr.append(at)
        if ln > K:
            ctx.check(ctx.lib.pc_hip_poly_div_multi(ctx.h, pc.CURVES[CURVE], C.c_void_p(p), 1, ln, C.c_void_p(pts.ctypes.data), K,
                                                    C.c_void_p(at), 1, C.c_void_p(rem.ctypes.data)))
        at += 32 * max(ln - K, 0)
    comb = torch.empty((m, 4), dtype=torch.int64, device="cuda")
    ctx.fr_lincomb(CURVE, qptr, etas, n_out=m, out=comb.data_ptr(), lens=[max(ln - K, 0) for ln in lens])
    res = alternate({"open_folding": lambda: srs.kzg_open_folding(poly.data_ptr(), rhos, pts, etas, n=n),
                     "final_msm": lambda: srs.msm(comb.data_ptr(), n=m, montgomery=True)})
    proof = srs.kzg_open_folding(poly.data_ptr(), rhos, pts, etas, n=n)[1]
    assert (proof == srs.msm(comb.data_ptr(), n=m, montgomery=True)[0]).all(), "the step-by-step scalars are not the call's"
    call, msm = res["open_folding"], res["final_msm"]
    print(json.dumps({"what": "open_folding", "log_n": log_n, "k": K, "open_folding_ms": call, "final_msm_ms": msm,
                      "folds_divisions_combination_ms": round(call[0] - msm[0], 3), "fraction_of_msm": round((call[0] - msm[0]) / msm[0], 3),
                      "launches_tree_and_rest": ctx.last_skzg_launches()}), flush=True)
    srs.free()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [20, 24]
    ctx = pc.Context(0)
    for log_n in sizes:
        run(ctx, log_n)
    ctx.close()


if __name__ == "__main__":
    main()
