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
Timing needs a GPU: there is no fallback.  Prints one JSON line per measurement and a Markdown table.

`--setup [nv ..]` (default 16 20 22) times the parameters instead, on TRUE keys made by pc_hip_ml_setup from a random trapdoor:
  - pc_hip_ml_setup as a whole and its host-bracketed phases (eq table, G1 level 0, G2 level 0, upper levels; timing on);
  - G2 against G1 fixed-base multiplications per second at equal n = 2^nv (pc_hip_g2_fixed_base_batch_mul and
    pc_hip_fixed_base_batch_mul on the same eq table, alternating);
  - pc_hip_ml_trim, and pc_hip_ml_open on the trimmed key (a real key, not a periodic one);
  - up to nv = 20, the only way to a resident pair-sum key without pc_hip_ml_setup: the levels on the host (read back from the
    device key here; making them is not counted) uploaded and reduced by multilinear_pair_key -- the ratios to pc_hip_ml_trim alone
    and to setup + trim, each with the run's minimum and maximum."""
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


def setup_leg(sizes):
    ctx = pc.Context(0)
    g = np.frombuffer(G.point_bytes(G.g1_generator(), True), dtype=np.uint8).copy()
    h = np.frombuffer(G.point_bytes(G.generator()), dtype=np.uint8).copy()
    rows = []
    for nv in sizes:
        n = 1 << nv
        reps = 5
        rng = np.random.default_rng(100 + nv)
        t = random_fr(rng, nv)
        ctx.set_timing(True)
        totals, phases = [], []
        keys = None
        for it in range(reps + 1):                          # the first pass is the warm-up (workspace, staging)
            if keys:
                keys[0].free(); keys[1].free()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            keys = ctx.ml_setup(CURVE, nv, g, h, t)[:2]
            ms = (time.perf_counter() - t0) * 1e3
            if it:
                totals.append(ms); phases.append(ctx.last_msm_phases_ms()[:4])
        ctx.set_timing(False)
        gk, hk = keys
        ph = [statistics.median(p[i] for p in phases) for i in range(4)]
        # fixed-base rates at equal n, alternating, on the same scalars
        eq = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        ctx.ml_eq_evals(CURVE, t, nv, eq.data_ptr())
        o1 = torch.empty((n, 12), dtype=torch.int64, device="cuda")
        o2 = torch.empty((n, 24), dtype=torch.int64, device="cuda")
        f1 = lambda: ctx.fixed_base_batch_mul(CURVE, g.view(np.uint64), eq.data_ptr(), n, o1.data_ptr())
        f2 = lambda: ctx.g2_fixed_base_batch_mul(CURVE, h, eq.data_ptr(), n, o2.data_ptr())
        f1(); f2()
        t1, t2 = [], []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); f2(); t2.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize(); t0 = time.perf_counter(); f1(); t1.append((time.perf_counter() - t0) * 1e3)
        del eq, o1, o2
        g1_ms, g2_ms = statistics.median(t1), statistics.median(t2)
        # trim and open on the real key
        made = []

        def trim():
            for k in made:
                k.free()
            made[:] = ctx.ml_trim(gk, hk, nv, nv)
        trm = stats(trim, 1, reps)
        ev = torch.from_numpy(random_fr(rng, n).view(np.int64)).cuda()
        pt = random_fr(rng, nv)
        opn = stats(lambda: made[1].ml_open(ev, nv, pt), 2, reps)
        rec = dict(kind="setup", nv=nv, setup_ms=statistics.median(totals), setup_min_max_ms=(min(totals), max(totals)), eq_table_ms=ph[0], g1_level0_ms=ph[1],
                   g2_level0_ms=ph[2], upper_levels_ms=ph[3], g1_fixed_base_ms=g1_ms, g1_min_max_ms=(min(t1), max(t1)), g2_fixed_base_ms=g2_ms,
                   g2_min_max_ms=(min(t2), max(t2)), g1_mul_per_s=n / g1_ms * 1e3, g2_mul_per_s=n / g2_ms * 1e3, ratio_g2_over_g1=g2_ms / g1_ms,
                   trim_ms=trm[0], trim_min_max_ms=trm[1:], open_real_key_ms=opn[0], open_min_max_ms=opn[1:])
        if nv <= 20:
            levels = [hk.read(pc.ml_level_offset(nv, i), n >> i) for i in range(nv)]
            old = []

            def upload():
                for k in old:
                    k.free()
                old[:] = [pc.multilinear_pair_key(ctx, CURVE, levels)]
            upl = stats(upload, 1, 3)
            same = old[0].read(0, n - 1).tobytes() == made[1].read(0, n - 1).tobytes()
            old[0].free()
            del levels
            rec.update(upload_pair_key_ms=upl[0], upload_min_max_ms=upl[1:], keys_equal=same, upload_over_trim=upl[0] / trm[0],
                       upload_over_trim_min_max=(upl[1] / trm[2], upl[2] / trm[1]), upload_over_setup_plus_trim=upl[0] / (rec["setup_ms"] + trm[0]),
                       upload_over_setup_plus_trim_min_max=(upl[1] / (max(totals) + trm[2]), upl[2] / (min(totals) + trm[1])))
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        for k in made + [gk, hk]:
            k.free()
        del ev
        torch.cuda.empty_cache()
        ctx.trim()
    ctx.close()
    print("\n| nv | setup ms (min-max) | eq table | G1 level 0 | G2 level 0 | upper levels | G1 mul/s | G2 mul/s | G2 / G1 | trim ms | open ms (real key) | upload + pair sums ms | / trim | / (setup + trim) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        tail = (f"{r['upload_pair_key_ms']:.1f} | {r['upload_over_trim']:.0f} | {r['upload_over_setup_plus_trim']:.2f} ({r['upload_over_setup_plus_trim_min_max'][0]:.2f}-{r['upload_over_setup_plus_trim_min_max'][1]:.2f})"
                if "upload_pair_key_ms" in r else "- | - | -")
        print(f"| {r['nv']} | {r['setup_ms']:.2f} ({r['setup_min_max_ms'][0]:.2f}-{r['setup_min_max_ms'][1]:.2f}) | {r['eq_table_ms']:.2f} | {r['g1_level0_ms']:.2f} | {r['g2_level0_ms']:.2f} | "
              f"{r['upper_levels_ms']:.2f} | {r['g1_mul_per_s']:.3g} | {r['g2_mul_per_s']:.3g} | {r['ratio_g2_over_g1']:.2f} | {r['trim_ms']:.2f} | {r['open_real_key_ms']:.2f} | {tail} |")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--open-only":
        return open_only(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
    if len(sys.argv) > 1 and sys.argv[1] == "--setup":
        return setup_leg([int(x) for x in sys.argv[2:]] or [16, 20, 22])
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
