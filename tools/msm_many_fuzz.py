"""Randomised differential test of the G1 many-MSM mode -- pc_hip_msm_many and the fast path of pc_hip_msm_batch -- against an
expectation made of Python integers: `python tools/msm_many_fuzz.py [seconds] [seed] [--curves a,b] [--case CASE_SEED] [--reference-only]`.

Per case: a curve, a key with known logarithms and both signs (tests/harness/signedkey.py: signed with or without holes, unsigned, one
base), a base offset, and B rows of m scalars, every row with a layout of its own: the cancelling layouts of signedkey (const,
pairwise, pairwise_few, all_but_one, opposite_scalars -- laid against the key positions the row meets) mixed with the distributions of
tools/msm_fuzz.py (uniform, a few values, all equal, runs, sparse, small, mixed, zeros).  Sizes: m in [1, 300] or [300, 6000] with
B in [1, 12] through pc_hip_msm_many (capped so that the pass stays below 2^21 entries at the narrowest window, 32 digits per scalar);
or, one case in six, m in [2^14, 2^14 + 2000] with 2 .. 4 polynomials through pc_hip_msm_batch over the key's window table (plain or GLV
form) under a chunk length of 0 (automatic), 1, 2, 5 or 8 -- 2^14 is the shortest length that takes the fast path, and only that path
honours the chunk length.  Scalars canonical or Montgomery, host or device memory.

The expected row is (sum_j s_j e_j mod r) G with e_j the key's logarithms: one scalar multiplication per row, all-zero words and the
infinity flag where the sum is 0 mod r.  Neither the device nor the oracle's bucket method has a part in it.

Prints one line per mismatch with the case's own seed (`--case CASE_SEED` replays exactly that case) and the summary
`msm_many_fuzz: N cases, M mismatches`; exit code 1 on any mismatch.  `--reference-only` leaves the device out (nothing is compared):
the rate of the harness side alone, which bounds what a slice of the suite can be asked for.  Measured over all four curves in ten
seconds: 310 cases on one CPU core without the device, 302 cases (47 of them batches) on an MI355X with the device in the loop --
tests/test_msm_cancel_gpu.py asks its ten-second slice for at least 75, under half of the smaller count."""
import os, sys, time, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import ctypes as C
import numpy as np
from harness import signedkey as SK

KEYS = ("signed", "signed_holes", "unsigned", "one_base")
KINDS = SK.LAYOUTS + ("uniform", "few", "equal", "runs", "sparse", "small", "mixed", "zeros")
BATCH_MIN = 1 << 14
ENTRY_CAP, MAX_DIGITS = 1 << 21, 32


def make_key(curve, kind, n):
    if kind == "signed": return SK.signed(curve, n)
    if kind == "signed_holes": return SK.signed(curve, n, holes=True)
    if kind == "unsigned": return SK.unsigned(curve, n)
    return SK.one_base(curve, n)


def make_row(rng, curve, kind, m, off, holes):
    r = SK.modulus(curve)
    if kind in SK.LAYOUTS:
        return SK.layout(kind, curve, m, rng.getrandbits(30), off, holes)
    if kind == "zeros": return [0] * m
    if kind == "equal": return [rng.randrange(r)] * m
    if kind == "few":
        v = [rng.randrange(r) for _ in range(rng.randint(2, 9))]
        return [v[i % len(v)] for i in range(m)]
    if kind == "runs":
        run = rng.randint(2, 4000); v = [rng.randrange(r) for _ in range(m // run + 1)]
        return [v[i // run] for i in range(m)]
    src = [rng.randrange(r) for _ in range(m)]
    if kind == "sparse":
        step = rng.randint(2, 50)
        return [v if i % step == 0 else 0 for i, v in enumerate(src)]
    if kind == "small":
        mask = (1 << rng.choice([64, 80])) - 1
        return [v & mask for v in src]
    if kind == "mixed": return [src[i % 7] if i % 3 == 0 else v for i, v in enumerate(src)]
    return src


def make_case(case_seed, curves):
    """everything of one case from its own seed: (parameters, key, rows of integers)"""
    rng = random.Random(case_seed)
    curve = rng.choice(curves)
    branch = rng.choice(["small", "small", "medium", "medium", "medium", "batch"])
    if branch == "batch":
        m, B = rng.randint(BATCH_MIN, BATCH_MIN + 2000), rng.randint(2, 4)
    else:
        m = rng.randint(1, 300) if branch == "small" else rng.randint(300, 6000)
        B = min(rng.randint(1, 12), max(1, (ENTRY_CAP - 1) // (m * MAX_DIGITS)))
    off = rng.choice([0, 0, 1, 5, 7, rng.randint(1, 200)])
    kkind = rng.choice(KEYS)
    key = make_key(curve, kkind, m + off)
    rows = []
    kinds = []
    for _ in range(B):
        kind = rng.choice(KINDS)
        if rows and rng.random() < 0.15:
            kind, row = "copy", list(rows[rng.randrange(len(rows))])
        else:
            row = make_row(rng, curve, kind, m, off, kkind == "signed_holes")
        rows.append(row); kinds.append(kind)
    prm = dict(curve=curve, m=m, B=B, off=off, key=kkind, rows=kinds, batch=branch == "batch", mont=rng.random() < 0.5, device=rng.random() < 0.5,
               T=rng.choice([0, 0, 1, 2, 5, 8]) if branch == "batch" else 0, glv=rng.random() < 0.4)
    return prm, key, rows


def device(ctx, prm, key, rows):
    """the rows through the entry point of the case: ((B, 2N) words, B flags)"""
    import torch
    from poly_commit_amd import _ffi
    curve, m, B, off = prm["curve"], prm["m"], prm["B"], prm["off"]
    arrs = [SK.mont(curve, r) if prm["mont"] else SK.limbs(r) for r in rows]
    ctx.set_msm_tuning(0, prm["T"])
    srs = ctx.upload_srs(curve, key.bases)
    try:
        if not prm["batch"]:
            mat = np.ascontiguousarray(np.stack(arrs))
            if prm["device"]:
                dev = torch.from_numpy(mat.view(np.int64)).cuda()
                return srs.msm_many(dev.data_ptr(), m=m, n_msms=B, base_offset=off, montgomery=prm["mont"])
            return srs.msm_many(mat, base_offset=off, montgomery=prm["mont"])
        srs.precompute(min_pairs=1, glv=prm["glv"])
        dev = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrs] if prm["device"] else None
        ptrs = (C.c_void_p * B)(*([t.data_ptr() for t in dev] if dev else [a.ctypes.data for a in arrs]))
        out = np.zeros((B, key.bases.shape[1]), dtype=np.uint64)
        infs = (C.c_int * B)()
        ctx.check(ctx.lib.pc_hip_msm_batch(ctx.h, srs.h, (C.c_size_t * B)(*[off] * B), ptrs, (C.c_size_t * B)(*[m] * B), B,
                                           _ffi.PC_SCALARS_MONTGOMERY if prm["mont"] else _ffi.PC_SCALARS_CANONICAL,
                                           _ffi.PC_MEM_DEVICE if prm["device"] else _ffi.PC_MEM_HOST, C.c_void_p(out.ctypes.data), infs))
        return out, np.array(list(infs), dtype=bool)
    finally:
        srs.free()
        ctx.set_msm_tuning(0, 0)


def main(argv):
    curves = tuple(SK.CURVES)
    if "--curves" in argv:
        i = argv.index("--curves")
        curves = tuple(argv[i + 1].split(","))
        del argv[i:i + 2]
    assert curves and all(c in SK.CURVES for c in curves), curves
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
    ctx = None
    if not ref_only:
        import poly_commit_amd as pc
        ctx = pc.Context(0)
    for c in curves:
        SK.pool(c)                                                               # (the pools before the clock starts)
    t0, cases, bad, batches = time.time(), 0, 0, 0
    while time.time() - t0 < budget:
        case_seed = one if one is not None else rng.getrandbits(32)
        prm, key, rows = make_case(case_seed, curves)
        want = np.stack([SK.expected(key, r, prm["off"]) for r in rows])
        cases += 1
        batches += prm["batch"]
        if ctx is not None:
            got, inf = device(ctx, prm, key, rows)
            if not ((got == want).all() and list(inf) == [not w.any() for w in want]):
                bad += 1
                print("MISMATCH --case", case_seed, prm, "rows that differ", [k for k in range(prm["B"]) if not (got[k] == want[k]).all()], flush=True)
        if one is not None:
            break
    print(f"msm_many_fuzz: {cases} cases, {bad} mismatches ({batches} through the batch fast path)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
