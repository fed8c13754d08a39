"""Randomised differential test of pc_hip_g2_msm against the pure-Python reference tests/harness/g2ref.py, bit-exact on the affine
Montgomery bytes.  `python tools/g2_msm_fuzz.py [seconds] [seed] [--case CASE_SEED] [--reference-only]`

Per case: n <= 2^15 pairs, a window width c in {0 (automatic), 4 .. 16}, a chunk length T in {0 (automatic), 1 .. 64}, one scalar
distribution (uniform, a few values, all equal, runs, sparse, runs of whole 128-lane workgroups), canonical or Montgomery scalars,
sometimes a base offset.  The key is periodic, H[x] = pool[x mod 64] (the pool holds the infinity, a repeated point and a P / -P
pair), so the expected point is ONE 64-point Python MSM of the scalars summed per residue: the reference is the cheap side.  One
process, one context; the key (and with it its pipeline, which takes the tuning when it is made) is freed after every case.

Prints one line per failure with the case's own seed (`--case CASE_SEED` replays exactly that case) and the summary
`g2_msm_fuzz: N cases, M mismatches`; exit code 1 on any mismatch.

`--reference-only` leaves the device out (nothing is compared): the rate of the Python side alone.  Measured on one CPU core:
90 cases in 10 s (9 cases/s; with the device in the loop an MI355X run made 154 cases in 10 s on a faster host) -- tests/test_g2_msm_gpu.py asks its ten-second slice for at least 20."""
import os, sys, time, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from harness import g2ref as G

CURVE = "bls12_381"
POOL = 64
NMAX = 1 << 15
KINDS = ("uniform", "few", "equal", "runs", "sparse", "wg_runs")


def make_pool():
    ks = [(i * 0x9e3779b97f4a7c15 + 0xf022) ** 3 % G.R for i in range(POOL)]
    p = G.fixed_base(G.generator()).mul_many(ks)
    p[5] = G.INF
    p[11] = p[10]
    p[21] = G.neg(p[20])
    return p


def make_case(case_seed):
    """everything of one case from its own seed: (parameters, canonical scalars as n x 32 bytes)"""
    rng = random.Random(case_seed)
    n = rng.choice([rng.randint(1, 300), rng.randint(300, 5000), rng.randint(5000, NMAX)])
    c = rng.choice([0, 0] + list(range(4, 17)))
    T = rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 16, 40, rng.randint(1, 64)])
    kind = rng.choice(KINDS)
    mont = rng.random() < 0.5
    off = rng.randint(1, 200) if rng.random() < 0.3 else 0
    src = np.frombuffer(np.random.RandomState(case_seed).bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    src[:, 31] &= 0x3f                                                          # canonical: below 2^254 < r
    idx = np.arange(n)
    if kind == "uniform": sc, par = src, 0
    elif kind == "few": par = rng.randint(2, 9); sc = src[idx % par]
    elif kind == "equal": par = 0; sc = np.repeat(src[:1], n, axis=0)
    elif kind == "runs": par = rng.randint(2, 4000); sc = src[idx // par]
    elif kind == "sparse": par = rng.randint(2, 50); sc = np.where((idx % par == 0)[:, None], src, 0).astype(np.uint8)
    else: par = 128 * rng.randint(1, 4); sc = src[idx // par]
    return dict(n=n, c=c, T=T, kind=kind, par=par, mont=mont, off=off), np.ascontiguousarray(sc)


def expected(pool, prm, sc):
    per = [0] * POOL
    for x, row in enumerate(sc):
        per[(x + prm["off"]) % POOL] += int.from_bytes(row.tobytes(), "little")
    return G.msm(pool, [v % G.R for v in per])


def device(ctx, pool_arr, prm, sc):
    n, off = prm["n"], prm["off"]
    bases = np.ascontiguousarray(np.tile(pool_arr, ((n + off + POOL - 1) // POOL, 1))[:n + off])
    if prm["mont"]:
        sc = G.scalars_array([int.from_bytes(row.tobytes(), "little") for row in sc], True)
    ctx.set_msm_tuning(prm["c"], prm["T"])
    key = ctx.upload_g2_srs(CURVE, bases)
    try:
        out, inf = key.msm(sc, base_offset=off, montgomery=prm["mont"])
        shape = ctx.last_msm_shape()
    finally:
        key.free()
        ctx.set_msm_tuning(0, 0)
    return G.point_from_bytes(out.tobytes()), inf, shape["window_bits"]


def main(argv):
    ref_only = "--reference-only" in argv
    if ref_only:
        argv.remove("--reference-only")
    one = None
    if "--case" in argv:
        i = argv.index("--case")
        one = int(argv[i + 1])
        del argv[i:i + 2]
    budget = float(argv[0]) if len(argv) > 0 else 60.0
    rng = random.Random(int(argv[1]) if len(argv) > 1 else 1)
    pool = make_pool()
    pool_arr = G.points_array(pool)
    ctx = None
    if not ref_only:
        import poly_commit_amd as pc
        ctx = pc.Context(0)
    t0, cases, bad = time.time(), 0, 0
    while time.time() - t0 < budget:
        case_seed = one if one is not None else rng.getrandbits(32)
        prm, sc = make_case(case_seed)
        want = expected(pool, prm, sc)
        cases += 1
        if ctx is not None:
            got, inf, c_ran = device(ctx, pool_arr, prm, sc)
            ok = got == want and inf == (want is G.INF) and (prm["c"] == 0 or c_ran == prm["c"])
            if not ok:
                bad += 1
                print("MISMATCH --case", case_seed, prm, "window bits of the call", c_ran, flush=True)
        if one is not None:
            break
    print(f"g2_msm_fuzz: {cases} cases, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
