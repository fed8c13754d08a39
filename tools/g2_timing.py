"""Time the G2 MSM and MultilinearPC's open on the device, beside a TABLE-FREE G1 MSM of the same lengths in the same run.

Per nv in {16, 20, 24} (or the sizes given): keys of 2^nv - 1 points (the length of an opening's pair-sum key), then
  - a blocking pc_hip_g2_msm over the whole key, scalars resident (canonical), and a blocking table-free pc_hip_msm on G1 over as many
    pairs -- warm-up, then the median / min / max of the repeats, the two alternating; their ratio (expected near 2.8: a G2 mixed
    addition is 56 product-or-reduction units with fused pairs, a G1 one 20);
  - pc_hip_ml_open (evaluations resident), split into the nv halving rounds alone (pc_hip_ml_fold driven one by one), the G2 MSMs of
    the rounds above the small-round threshold (pc_hip_g2_msm per round) and the rest (small rounds, copies, host tails);
  - the open of the smallest size in child processes with other values of PC_HIP_G2_SMALL_ROUND (read once per process).
Keys are made of DISTINCT points without a device-side fixed-base multiplication: two pools of 2^12 Python-made points, point (a, b) of
the key = P_a + Q_b by pc_hip_g2_srs_pair_sums (a periodic key would put equal points into one bucket and time the doubling branch).
Timing needs a GPU: there is no fallback.  Prints one JSON line per measurement and a Markdown table."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import oracle_lib as O  # noqa: E402
import poly_commit_amd as pc  # noqa: E402
from harness import g2ref as G  # noqa: E402

CURVE = "bls12_381"
POOL = 1 << 12


def pools(path):
    if not os.path.exists(path):
        fb = G.fixed_base(G.generator())
        ka = [(i * 0x9e3779b97f4a7c15 + 0x51) ** 3 % G.R for i in range(POOL)]
        kb = [(i * 0xc2b2ae3d27d4eb4f + 0x77) ** 5 % G.R for i in range(POOL)]
        np.savez(path, a=G.points_array(fb.mul_many(ka)), b=G.points_array(fb.mul_many(kb)))
    d = np.load(path)
    return d["a"], d["b"]


def make_g2_key(ctx, n, pa, pb):
    """n distinct points: key[x] = P[x mod 2^12] + Q[x div 2^12], built on the device in slabs of 2^19 pairs"""
    key = pc.G2Srs(ctx, CURVE, np.zeros((n, 192), dtype=np.uint8))
    slab = 1 << 19
    for first in range(0, n, slab):
        cnt = min(slab, n - first)
        x = np.arange(first, first + cnt)
        both = np.empty((2 * cnt, 192), dtype=np.uint8)
        both[0::2] = pa[x % POOL]
        both[1::2] = pb[(x // POOL) % POOL]
        lvl = pc.G2Srs(ctx, CURVE, both)
        lvl.pair_sums_into(key, 0, cnt, first)
        lvl.free()
    return key


def stats(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                    # the calls block: they return with the result on the host
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def random_fr(rng, n):
    v = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 61) - 1)        # below 2^253 < r: canonical scalars / valid Montgomery residues
    return v


def open_only(nv, pool_path, reps):
    pa, pb = pools(pool_path)
    ctx = pc.Context(0)
    n = 1 << nv
    key = make_g2_key(ctx, n - 1, pa, pb)
    rng = np.random.default_rng(nv)
    ev = torch.from_numpy(random_fr(rng, n).view(np.int64)).cuda()
    pt = random_fr(rng, nv)
    m = stats(lambda: key.ml_open(ev, nv, pt), 2, reps)
    print(json.dumps(dict(kind="open_threshold", nv=nv, small_round=os.environ.get("PC_HIP_G2_SMALL_ROUND", "default"), open_ms=m[0], min_max_ms=m[1:])), flush=True)
    key.free()
    ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--open-only":
        return open_only(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
    sizes = [int(x) for x in sys.argv[1:]] or [16, 20, 24]
    pool_path = os.path.join(tempfile.mkdtemp(prefix="g2_timing_"), "pools.npz")
    pa, pb = pools(pool_path)
    small = int(os.environ.get("PC_HIP_G2_SMALL_ROUND", "32"))
    ctx = pc.Context(0)
    rows = []
    for nv in sizes:
        n = 1 << nv
        reps = 5 if nv >= 24 else 9
        rng = np.random.default_rng(nv)
        key = make_g2_key(ctx, n - 1, pa, pb)
        g1 = ctx.upload_srs(CURVE, O.gen_bases(CURVE, n - 1))          # no window table: table-free
        sc = torch.from_numpy(random_fr(rng, n - 1).view(np.int64)).cuda()
        # alternate the two inside one loop: the same clocks, the same neighbours
        key.msm(sc, n=n - 1); g1.msm(sc, n=n - 1); key.msm(sc, n=n - 1); g1.msm(sc, n=n - 1)
        t2, t1 = [], []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); key.msm(sc, n=n - 1); t2.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize(); t0 = time.perf_counter(); g1.msm(sc, n=n - 1); t1.append((time.perf_counter() - t0) * 1e3)
        g2_ms, g1_ms = statistics.median(t2), statistics.median(t1)
        g1.free()
        ev = torch.from_numpy(random_fr(rng, n).view(np.int64)).cuda()
        pt = random_fr(rng, nv)
        opn = stats(lambda: key.ml_open(ev, nv, pt), 2, reps)
        # the halving rounds alone
        bufs = [torch.empty((n // 2, 4), dtype=torch.int64, device="cuda"), torch.empty((max(n // 4, 1), 4), dtype=torch.int64, device="cuda")]
        q = torch.empty((n // 2, 4), dtype=torch.int64, device="cuda")

        def folds():
            r = ev
            for i in range(nv):
                out = bufs[i & 1]
                ctx.ml_fold(CURVE, r.data_ptr(), n >> (i + 1), pt[i], out.data_ptr(), q.data_ptr())
                r = out
        fold = stats(folds, 1, reps)
        # the MSMs of the rounds above the threshold (q of round 0 stands in for every round's scalars)
        ctx.ml_fold(CURVE, ev.data_ptr(), n // 2, pt[0], bufs[0].data_ptr(), q.data_ptr())

        def big_msms():
            for i in range(nv):
                half = n >> (i + 1)
                if half > small:
                    key.msm(q, n=half, base_offset=n - (n >> i), montgomery=True)
        msms = stats(big_msms, 1, reps)
        rec = dict(kind="sizes", nv=nv, pairs=n - 1, g2_msm_ms=g2_ms, g2_min_max_ms=(min(t2), max(t2)), g1_table_free_msm_ms=g1_ms, g1_min_max_ms=(min(t1), max(t1)),
                   ratio_g2_over_g1=g2_ms / g1_ms, open_ms=opn[0], open_min_max_ms=opn[1:], fold_rounds_ms=fold[0], msm_rounds_ms=msms[0],
                   small_rounds_and_rest_ms=opn[0] - fold[0] - msms[0], small_round_threshold=small)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        key.free()
        del ev, sc, q, bufs
        torch.cuda.empty_cache()
    ctx.close()
    for nv in sizes[:1]:                                # the late rounds are the same at every nv: the smallest size shows the threshold's effect
        for thr in ("0", "8", "32", "128"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--open-only", str(nv), pool_path, "9"], env=dict(os.environ, PC_HIP_G2_SMALL_ROUND=thr),
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(json.dumps(dict(kind="open_threshold", nv=nv, small_round=thr, error=r.stderr[-400:])), flush=True)
                break                                   # nothing more is started on the device after a failure
            print(r.stdout.strip().splitlines()[-1], flush=True)
    print("\n| nv | pairs | G2 MSM ms (min-max) | G1 table-free MSM ms (min-max) | G2 / G1 | ml_open ms | folds ms | MSM rounds ms | small rounds + rest ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['nv']} | {r['pairs']} | {r['g2_msm_ms']:.2f} ({r['g2_min_max_ms'][0]:.2f}-{r['g2_min_max_ms'][1]:.2f}) | {r['g1_table_free_msm_ms']:.2f} ({r['g1_min_max_ms'][0]:.2f}-{r['g1_min_max_ms'][1]:.2f}) | "
              f"{r['ratio_g2_over_g1']:.2f} | {r['open_ms']:.2f} | {r['fold_rounds_ms']:.2f} | {r['msm_rounds_ms']:.2f} | {r['small_rounds_and_rest_ms']:.2f} |")


if __name__ == "__main__":
    main()
