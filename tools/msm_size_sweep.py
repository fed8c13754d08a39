"""Blocking MSM latency vs size (device-resident scalars, key trimmed to the size, with and without its window table):
wall clock per call, the hipEvent phase brackets of the last call (digits+histogram, scan, scatter+fine sort, accumulate,
segmented reduction, bucket reduction) and the plan's shape {window bits, digits per scalar, buckets, table used}."""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import oracle_lib as O
import poly_commit_amd as pc
ctx = pc.Context(0)
ctx.set_timing(True)
if os.environ.get("PC_SWEEP_CHUNK"): ctx.set_msm_tuning(0, int(os.environ["PC_SWEEP_CHUNK"]))
out = {}
curves = os.environ.get("PC_SWEEP_CURVES", "bls12_381").split(",")
sizes = [int(x) for x in os.environ.get("PC_SWEEP_LOGS", "8,10,12,14,16,18,20").split(",")]
def device_made_inputs(curve, nmax):
    """A curve the CPU oracle does not have (BLS12-377): the bases are k_i G for seeded random k_i, made on the device by
    pc_hip_fixed_base_batch_mul; the scalars are seeded random residues below 2^252 < r, taken as Montgomery forms."""
    from harness import ref377 as B
    assert curve == B.CURVE
    rng = np.random.default_rng(3)
    def residues():
        a = rng.integers(0, 1 << 63, size=(nmax, 4), dtype=np.int64)
        a[:, 3] &= (1 << 60) - 1
        return torch.from_numpy(a).cuda()
    ks = residues()
    pts = torch.empty((nmax, 12), dtype=torch.int64, device="cuda")
    ctx.fixed_base_batch_mul(curve, B.point(B.G), ks.data_ptr(), nmax, pts.data_ptr())
    torch.cuda.synchronize()
    return pts.data_ptr(), residues(), pts


for curve in curves:
    nmax = 1 << max(sizes)
    if curve in O.pyref.CURVES:
        bases = O.gen_bases(curve, nmax)
        sc = torch.from_numpy(O.f_to_mont(curve, 1, O.gen_scalars(curve, 3, nmax)).view(np.int64)).cuda()
    else:
        bases, sc, keep = device_made_inputs(curve, nmax)
    torch.cuda.synchronize()
    row = {}
    for lg in sizes:
        n = 1 << lg
        for table in (False, True):
            srs = ctx.upload_srs(curve, bases, n=n)
            if table: srs.precompute()
            for _ in range(3): srs.msm(sc.data_ptr(), n=n, montgomery=True)
            reps = 20
            t = time.perf_counter()
            for _ in range(reps): srs.msm(sc.data_ptr(), n=n, montgomery=True)
            ms = (time.perf_counter() - t) / reps * 1e3
            ph = ctx.last_msm_phases_ms()
            row[f"2^{lg}" + ("+table" if table else "")] = {"ms": round(ms, 3), "phases": [round(x, 3) for x in ph[:6]],
                                                           "sum_phases": round(sum(ph[:6]), 3), "shape": ctx.last_msm_shape()}
            srs.free()
    out[curve] = row
print(json.dumps(out))
