"""Time the twisted Edwards MSM (pc_hip_te_msm) and key fold (pc_hip_te_ec_fold) on the device, beside a TABLE-FREE BN254 pc_hip_msm of the
same lengths in the same process -- the other curve with 8-word coordinates.

Per log2 n in {16, 20, 22} (or the sizes given):
  - a blocking pc_hip_te_msm over n pairs, scalars resident (canonical), and a blocking table-free BN254 pc_hip_msm on resident scalars
    over as many pairs: warm-up, then 7 repeats of each, the two ALTERNATING; median with minimum and maximum, and the ratio of the
    medians with the ratio's own range.  By multiplication count the bucket accumulation should take about 0.7 of BN254's (7M against
    8M + 2S); the ratio is reported with the phase brackets of both pipelines (pc_hip_last_msm_phases_ms) so that it can be explained.
  - pc_hip_te_ec_fold at n_half = 2^17 (one round of an opening over a 2^18-point key): each repeat folds the same key again (the fold
    is in place; its time does not depend on the values).
The comparison is against the BN254 run on the same box, not against a fixed figure.
TE keys are made of DISTINCT points without Python making 2^22 of them: two pools of 2^12 Python-made multiples of G, the lower half
of a 2n-point key tiled from the first, the upper half from the second, one pc_hip_te_ec_fold with u = 1: key[x] = P[x mod 2^12] +
Q[x div 2^12] (a periodic key would put equal points into one bucket).  Timing needs a GPU: there is no fallback.  Prints one JSON
line per measurement and a Markdown table."""
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
from harness import teref as E  # noqa: E402

TE, G1 = "ed_on_bls12_381", "bn254"
POOL = 1 << 12
REPS = 7
PHASES = ("stage_digits", "scans", "scatter_fine", "accumulate", "seg_reduce", "bucket_reduce")      # the brackets between a pipeline's marks (msm.hpp)


def pools():
    fb = E.fixed_base(E.GEN)
    ka = [(i * 0x9e3779b97f4a7c15 + 0x51) ** 3 % E.R for i in range(POOL)]
    kb = [(i * 0xc2b2ae3d27d4eb4f + 0x77) ** 5 % E.R for i in range(POOL)]
    return E.points_array(fb.mul_many(ka)), E.points_array(fb.mul_many(kb))


def make_te_key(ctx, n, pa, pb):
    """2n resident points whose first n are distinct: key[x] = P[x mod 2^12] + Q[x div 2^12] by one fold with u = 1"""
    x = np.arange(n)
    both = np.empty((2 * n, 64), dtype=np.uint8)
    both[:n] = pa[x % POOL]
    both[n:] = pb[(x // POOL) % POOL]
    key = ctx.upload_te_srs(TE, both)
    key.ec_fold(n, E.scalars_array([1], True)[0])
    return key


def random_scalars(rng, n, bits):
    """canonical scalars below 2^bits (bits below the modulus' length)"""
    v = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << (bits - 192)) - 1)
    return v


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                        # the calls block: they return with the result on the host
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16, 20, 22]
    pa, pb = pools()
    ctx = pc.Context(0)
    rows = []
    for lg in sizes:
        n = 1 << lg
        rng = np.random.default_rng(lg)
        te_key = make_te_key(ctx, n, pa, pb)
        g1_key = ctx.upload_srs(G1, O.gen_bases(G1, n))          # no precompute(): table-free, as the TE pipeline is
        s_te = torch.from_numpy(random_scalars(rng, n, 251).view(np.int64)).cuda()
        s_g1 = torch.from_numpy(random_scalars(rng, n, 253).view(np.int64)).cuda()
        f_te = lambda: te_key.msm(s_te, n=n)
        f_g1 = lambda: g1_key.msm(s_g1, n=n)
        for _ in range(2):
            f_te(); f_g1()
        t_te, t_g1 = [], []
        for _ in range(REPS):
            t_te.append(timed(f_te))
            t_g1.append(timed(f_g1))
        # the phase brackets of one more call each (timing on adds event records: not part of the medians above)
        ctx.set_timing(True)
        f_te(); ph_te = ctx.last_msm_phases_ms()[:6]
        f_g1(); ph_g1 = ctx.last_msm_phases_ms()[:6]
        ctx.set_timing(False)
        m_te, m_g1 = med(t_te), med(t_g1)
        rec = dict(kind="msm", log2_n=lg, te_ms=m_te[0], te_min_max_ms=m_te[1:], bn254_ms=m_g1[0], bn254_min_max_ms=m_g1[1:],
                   ratio=m_te[0] / m_g1[0], ratio_min_max=(m_te[1] / m_g1[2], m_te[2] / m_g1[1]),
                   te_phases_ms=dict(zip(PHASES, ph_te)), bn254_phases_ms=dict(zip(PHASES, ph_g1)),
                   accumulate_ratio=(ph_te[3] / ph_g1[3]) if ph_g1[3] else None)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        te_key.free(); g1_key.free()
        del s_te, s_g1
        torch.cuda.empty_cache()
        ctx.trim()
    # the key fold: n_half = 2^17
    half = 1 << 17
    x = np.arange(2 * half)
    key = ctx.upload_te_srs(TE, np.ascontiguousarray(pa[x % POOL]))
    u = E.scalars_array([0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd % E.R], True)[0]
    fold = lambda: key.ec_fold(half, u)
    fold()
    m = med([timed(fold) for _ in range(REPS)])
    rec = dict(kind="ec_fold", n_half=half, ms=m[0], min_max_ms=m[1:], points_per_s=half / m[0] * 1e3)
    print(json.dumps(rec), flush=True)
    key.free()
    ctx.close()
    print("\n| log2 n | TE MSM ms (min-max) | BN254 table-free ms (min-max) | TE / BN254 (range) | accumulate TE / BN254 ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['log2_n']} | {r['te_ms']:.2f} ({r['te_min_max_ms'][0]:.2f}-{r['te_min_max_ms'][1]:.2f}) | {r['bn254_ms']:.2f} ({r['bn254_min_max_ms'][0]:.2f}-{r['bn254_min_max_ms'][1]:.2f}) | "
              f"{r['ratio']:.2f} ({r['ratio_min_max'][0]:.2f}-{r['ratio_min_max'][1]:.2f}) | {r['te_phases_ms']['accumulate']:.2f} / {r['bn254_phases_ms']['accumulate']:.2f} |")
    print(f"\npc_hip_te_ec_fold, n_half = 2^17: {rec['ms']:.2f} ms ({rec['min_max_ms'][0]:.2f}-{rec['min_max_ms'][1]:.2f}), {rec['points_per_s']:.3g} points/s")


if __name__ == "__main__":
    main()
