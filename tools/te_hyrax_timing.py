"""Time HyraxPC over ed_on_bls12_381 on the device (poly_commit_amd/te_hyrax.py): commit, open and check at num_vars 12, 16 and 20
(the reference's own Hyrax benchmark runs 12 to 22, benches/hyrax_times.rs:24-25), and in the same run, per shape:

  - the commit's rows as a loop of dim blocking pc_hip_te_msm calls over the same extended key and the same resident scalars -- what
    a caller had before pc_hip_te_msm_many.  The pass and the loop ALTERNATE inside one repeat loop; the pass must not be slower.
  - a BN254 pc_hip_msm_many of the same shape (dim MSMs of dim + 1 pairs), the other curve with 8-word coordinates: the ratio is
    reported, nothing is asserted about it.
  - the first pc_hip_te_msm_many call of the shape, which builds the window table and the pass's pipeline, and the table's bytes.

Method: every timed call blocks (it returns with the result on the host), a host clock around it after a device synchronise; two
warm-up rounds per shape, then the median of 5 with minimum and maximum.  open and check include their host work (the tensors of the
point, the singleton commitments, the verifier's two equations): they are the scheme's functions, not kernels.  The key is made of
known multiples of G (distinct points).  Timing needs a GPU: there is no fallback.  Prints one JSON line per shape and a Markdown
table; exits non-zero if the pass was slower than the loop at any shape."""
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
from poly_commit_amd import te_hyrax as T  # noqa: E402

TE, G1 = "ed_on_bls12_381", "bn254"
REPS = 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def random_fr(rng, shape, top_bits):
    """residues below 2^(224 + top_bits) as bytes: valid as canonical scalars and as Montgomery forms alike"""
    a = rng.integers(0, 256, size=tuple(shape) + (32,), dtype=np.uint8)
    a[..., 31] &= (1 << (top_bits - 24)) - 1
    return a


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [12, 16, 20]
    ctx = pc.Context(0)
    fb = E.fixed_base(E.GEN)
    rows, slower = [], []
    for nv in sizes:
        dim = 1 << (nv // 2)
        rng = np.random.default_rng(nv)
        kk = [(i * 0x9e3779b97f4a7c15 + 0x5eed) ** 3 % E.R for i in range(dim + 1)]
        key = T.TeHyraxKey(ctx, ctx.upload_te_srs(TE, E.points_array(fb.mul_many(kk))), nv)
        evals = torch.from_numpy(random_fr(rng, (1 << nv,), 27)).cuda()
        rands = random_fr(rng, (dim,), 27)
        point, d = random_fr(rng, (nv,), 27), random_fr(rng, (dim,), 27)
        r_eval, r_d, r_b, c = random_fr(rng, (4,), 27)
        # the first call of the shape: window table + the pass's pipeline + the pass
        first_ms = timed(lambda: T.commit(key, evals, rands))
        res = key.full.bytes_resident()
        shape = ctx.last_msm_shape()
        row_coms, state = T.commit(key, evals, rands)
        # the same rows as dim blocking single MSMs: the scalars row_i || r_i resident, as the pass reads them
        ext = torch.cat([state[1], torch.from_numpy(rands).cuda().view(dim, 1, 32)], dim=1).contiguous()
        base, step = ext.data_ptr(), (dim + 1) * 32
        loop_out = np.zeros((dim, 64), dtype=np.uint8)

        def loop():
            for i in range(dim):
                loop_out[i] = key.full.msm(base + i * step, n=dim + 1, montgomery=True)[0]
        g1 = ctx.upload_srs(G1, O.gen_bases(G1, dim + 1))
        s_g1 = torch.from_numpy(random_fr(rng, (dim, dim + 1), 29)).cuda()
        f_commit = lambda: T.commit(key, evals, rands)
        f_g1 = lambda: g1.msm_many(s_g1.data_ptr(), m=dim + 1, n_msms=dim)
        holder = {}

        def f_open():
            holder["proof"] = T.open(key, state, point, r_eval, d, r_d, r_b, c)[0]
        f_check = lambda: T.check(key, row_coms, point, holder["proof"], c)
        for _ in range(2):
            f_commit(); loop(); f_g1(); f_open(); assert f_check()
        assert (loop_out == row_coms).all()                      # the pass and the loop give the same points
        t = {k: [] for k in ("commit", "loop", "bn254", "open", "check")}
        for _ in range(REPS):
            t["commit"].append(timed(f_commit))
            t["loop"].append(timed(loop))
            t["bn254"].append(timed(f_g1))
            t["open"].append(timed(f_open))
            t["check"].append(timed(f_check))
        ctx.set_timing(True)
        f_commit(); ph = ctx.last_msm_phases_ms()[:6]
        ctx.set_timing(False)
        m = {k: med(v) for k, v in t.items()}
        rec = dict(kind="te_hyrax", num_vars=nv, dim=dim, window_bits=shape["window_bits"], windows=shape["digits_per_scalar"], buckets=shape["buckets"],
                   commit_ms=m["commit"][0], commit_min_max_ms=m["commit"][1:], loop_ms=m["loop"][0], loop_min_max_ms=m["loop"][1:],
                   loop_over_commit=m["loop"][0] / m["commit"][0], bn254_many_ms=m["bn254"][0], bn254_many_min_max_ms=m["bn254"][1:],
                   commit_over_bn254=m["commit"][0] / m["bn254"][0], open_ms=m["open"][0], open_min_max_ms=m["open"][1:],
                   check_ms=m["check"][0], check_min_max_ms=m["check"][1:], first_commit_ms=first_ms, table_and_pipeline_ms=first_ms - m["commit"][0],
                   table_bytes=res["window_tables"], pipeline_bytes=res["lanes"],
                   commit_phases_ms=dict(zip(("stage_digits", "scans", "scatter_fine", "accumulate", "seg_reduce", "bucket_reduce"), ph)))
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        if m["commit"][0] > m["loop"][0]:
            slower.append(nv)
        g1.free(); key.close()
        del evals, ext, s_g1, state
        torch.cuda.empty_cache()
        ctx.trim()
    ctx.close()
    print("\n| num_vars | commit ms (min-max) | loop of dim pc_hip_te_msm ms (min-max) | loop / commit | BN254 pc_hip_msm_many ms | commit / BN254 | open ms | check ms | first commit ms | table bytes |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['num_vars']} | {r['commit_ms']:.2f} ({r['commit_min_max_ms'][0]:.2f}-{r['commit_min_max_ms'][1]:.2f}) | "
              f"{r['loop_ms']:.2f} ({r['loop_min_max_ms'][0]:.2f}-{r['loop_min_max_ms'][1]:.2f}) | {r['loop_over_commit']:.1f} | {r['bn254_many_ms']:.2f} | "
              f"{r['commit_over_bn254']:.2f} | {r['open_ms']:.2f} | {r['check_ms']:.2f} | {r['first_commit_ms']:.2f} | {r['table_bytes']} |")
    if slower:
        print(f"\nthe many-MSM commit was SLOWER than the loop at num_vars {slower}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
