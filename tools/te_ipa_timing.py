"""Time the device path of InnerProductArgPC over ed_on_bls12_381: the key fold from the fold table against the ladder, a whole opening
through pc_hip_te_ipa_open_rounds against the sequence an integration had before it, and the two one-off costs per key.

  fold      n_half = 2^17 and 2^19: pc_hip_te_ec_fold (the in-place ladder, on a copy), pc_hip_te_ec_fold_from without a table (the same
            ladder, out of place) and with the key's table; one call each, the sides ALTERNATING, median of 7 with min and max.
            An out-of-place fold includes the allocation of its result key, on both sides alike.
  open      2^16 and 2^20 coefficients: pc_hip_te_ipa_open_rounds with fixed_key_below in 2^14 .. 2^17, with and without the key's fold
            table, against the PARENT SEQUENCE -- a working copy of the key, then per round two pc_hip_te_msm with scalars from the host and
            one pc_hip_te_ec_fold, which is all the device did for an opening before the call existed.  The Fr vectors of that sequence
            were folded on the host; that host arithmetic is LEFT OUT of the parent's time here (its scalars are random vectors of the
            round's length), so the parent's figure is a lower bound of what it cost.  Alternating, median of 7 with min and max, and
            the per-round and per-fold times of the new call's best form.
  one-off   pc_hip_te_srs_precompute_fold and pc_hip_te_srs_in_subgroup on a fresh key of each size (3 repeats, fresh key each).
The transcript of the timed openings is a fixed challenge schedule (a hash of two points per round is not what is measured).
Keys: the lower and upper halves tiled from two pools of 2^12 Python-made multiples of G and folded once with u = 1, as tools/te_timing.py
does.  Needs a GPU: there is no fallback.  Appends one JSON line per measurement to profiles/te_ipa_timing.jsonl and prints them."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import poly_commit_amd as pc  # noqa: E402
from harness import teref as E  # noqa: E402

TE = "ed_on_bls12_381"
POOL = 1 << 12
REPS = 7
OUT = os.path.join(ROOT, "profiles", "te_ipa_timing.jsonl")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def pools():
    fb = E.fixed_base(E.GEN)
    ka = [(i * 0x9e3779b97f4a7c15 + 0x51) ** 3 % E.R for i in range(POOL)]
    kb = [(i * 0xc2b2ae3d27d4eb4f + 0x77) ** 5 % E.R for i in range(POOL)]
    return E.points_array(fb.mul_many(ka)), E.points_array(fb.mul_many(kb))


def key_points(ctx, n, pa, pb):
    """n distinct subgroup points as a host array: key[x] = P[x mod 2^12] + Q[x div 2^12] by one fold with u = 1 on the device"""
    x = np.arange(n)
    both = np.empty((2 * n, 64), dtype=np.uint8)
    both[:n] = pa[x % POOL]
    both[n:] = pb[(x // POOL) % POOL]
    k = ctx.upload_te_srs(TE, both)
    k.ec_fold(n, E.scalars_array([1], True)[0])
    out = k.read(0, n)
    k.free()
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                        # the calls block
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def alternating(sides, reps=REPS, warm=2):
    """{name: fn} -> {name: [median, min, max]}: every repeat runs each side once, in turn"""
    for _ in range(warm):
        for fn in sides.values():
            fn()
    ts = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            ts[name].append(timed(fn))
    return {name: med(v) for name, v in ts.items()}


def rand_fr(rng, n):
    """n Montgomery-form scalars: any residue below 2^251 < r"""
    v = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    v[:, 31] &= 0x07
    return v


def challenge_schedule(seed):
    ks = [(seed * 0x9e3779b97f4a7c15 + i * 0xc2b2ae3d27d4eb4f + 0x1234567) ** 5 % E.R for i in range(32)]
    return [E.scalars_array([k], True)[0] for k in ks]


def time_folds(ctx, arr_of, lg_half):
    half = 1 << lg_half
    arr = arr_of(2 * half)
    plain, tabled, copy = ctx.upload_te_srs(TE, arr), ctx.upload_te_srs(TE, arr), ctx.upload_te_srs(TE, arr)
    t_build = timed(tabled.precompute_fold)
    u = challenge_schedule(lg_half)[0]
    sides = {"in_place_ladder": lambda: copy.ec_fold(half, u),                      # (folds the same key again: the time does not depend on the values)
             "from_ladder": lambda: plain.ec_fold_from(half, u).free(),
             "from_table": lambda: tabled.ec_fold_from(half, u).free()}
    res = alternating(sides)
    emit(dict(kind="fold", log2_n_half=lg_half, ms=res, table_over_in_place=round(res["from_table"][0] / res["in_place_ladder"][0], 4),
              table_over_from_ladder=round(res["from_table"][0] / res["from_ladder"][0], 4), table_build_ms=round(t_build, 3),
              table_bytes=tabled.bytes_resident()["fold_table"]))
    for k in (plain, tabled, copy):
        k.free()


def parent_sequence(ctx, arr, n, h_prime, rng):
    """what the device did for an opening before pc_hip_te_ipa_open_rounds: a working copy of the key, then per round two MSMs with host
    scalars, two host point multiplications and sums, and one in-place fold (the host's Fr folds are not timed: see the module text)"""
    scal = {m: (rand_fr(rng, m), rand_fr(rng, m)) for m in [n >> i for i in range(1, n.bit_length())]}
    dots = rand_fr(rng, 2)
    us = challenge_schedule(n)

    def run():
        work = ctx.upload_te_srs(TE, arr)
        m, rnd = n, 0
        while m > 1:
            h = m // 2
            ml, _ = work.msm(scal[h][0], n=h, base_offset=0, montgomery=True)
            mr, _ = work.msm(scal[h][1], n=h, base_offset=h, montgomery=True)
            pc.te_points_sum(TE, np.stack([ml, pc.te_point_mul(TE, h_prime, dots[0])]))
            pc.te_points_sum(TE, np.stack([mr, pc.te_point_mul(TE, h_prime, dots[1])]))
            work.ec_fold(h, us[rnd])
            m, rnd = h, rnd + 1
        work.read(0, 1)
        work.free()
    return run


def new_call(key, n, h_prime, rng, fkb, times=None):
    coeffs = torch.from_numpy(rand_fr(rng, n)).cuda()
    point = E.scalars_array([0x5555aaaa5555aaaa5555aaaa % E.R], True)[0]
    us = challenge_schedule(n)

    def run():
        work = coeffs.clone()                                                       # the call consumes its coefficients
        it = iter(us)
        out = key.ipa_open_rounds(work, n, point, h_prime, lambda l, r: next(it), fkb, want_times=times is not None)
        if times is not None:
            times["round_ms"], times["fold_ms"] = [round(x, 3) for x in out[4]], [round(x, 3) for x in out[5]]
    return run


def time_openings(ctx, arr_of, lg):
    n = 1 << lg
    arr = arr_of(n)
    rng = np.random.default_rng(lg)
    h_prime = E.points_array([E.mul(0x1234567, E.GEN)])[0]
    plain, tabled = ctx.upload_te_srs(TE, arr), ctx.upload_te_srs(TE, arr).precompute_fold()
    t_sub = timed(plain.in_subgroup)
    tabled.in_subgroup()
    sides = {"parent_sequence": parent_sequence(ctx, arr, n, h_prime, rng)}
    for lgf in (14, 15, 16, 17):
        sides["table_fkb_2^%d" % lgf] = new_call(tabled, n, h_prime, rng, 1 << lgf)
        sides["ladder_fkb_2^%d" % lgf] = new_call(plain, n, h_prime, rng, 1 << lgf)
    sides["table_fold_every_round"] = new_call(tabled, n, h_prime, rng, 1)
    res = alternating(sides, warm=1)
    best = min((k for k in res if k != "parent_sequence"), key=lambda k: res[k][0])
    times = {}
    lgf = int(best.split("^")[1]) if "^" in best else 0
    new_call(tabled if best.startswith("table") else plain, n, h_prime, rng, (1 << lgf) if lgf else 1, times)()
    emit(dict(kind="open", log2_n=lg, ms=res, best=best, best_over_parent=round(res[best][0] / res["parent_sequence"][0], 4),
              best_round_ms=times["round_ms"], best_fold_ms=times["fold_ms"], subgroup_check_ms=round(t_sub, 3)))
    plain.free()
    tabled.free()


def time_one_off(ctx, arr_of, lg):
    n = 1 << lg
    arr = arr_of(n)
    build, sub = [], []
    for _ in range(3):
        k = ctx.upload_te_srs(TE, arr)
        build.append(timed(k.precompute_fold))
        sub.append(timed(k.in_subgroup))
        k.free()
    emit(dict(kind="one_off", log2_n=lg, precompute_fold_ms=med(build), in_subgroup_ms=med(sub)))


def main():
    what = sys.argv[1:] or ["fold:17", "fold:19", "open:16", "open:20", "one_off:16", "one_off:20"]
    pa, pb = pools()
    ctx = pc.Context(0)
    cache = {}

    def arr_of(n):
        if n not in cache:
            cache.clear()
            cache[n] = key_points(ctx, n, pa, pb)
        return cache[n]
    for w in what:
        kind, lg = w.split(":")
        {"fold": time_folds, "open": time_openings, "one_off": time_one_off}[kind](ctx, arr_of, int(lg))
        torch.cuda.empty_cache()
        ctx.trim()
    ctx.close()


if __name__ == "__main__":
    main()
