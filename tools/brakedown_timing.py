"""Time the Brakedown encoder and commit on the device: BN254, default codes at num_vars 12..24 (the reference's benchmark,
poly-commit/benches/brakedown_ml_times.rs, runs 12..20), warm, median of the repeats.

Per size: encode alone (device to device), the four phases of pc_hip_brakedown_commit (timing on), the whole commit from and to host
memory.  Beside them the same encode on the host -- tests/cpp/brakedown_driver `time`, the C++ mirror's row_mul loop on 16 threads: a
PORT of the reference's algorithm, not the reference (which cannot be built here) -- and rows x non-zeros / encode time as a fraction
of the memory-free multiply rate of tools/microbench (fmul bn254_fr).  The matrices have the default shape and d random places per
row; their draw order does not matter for a timing.  Prints one JSON line per size and a Markdown table."""
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import poly_commit_amd as pc  # noqa: E402
from harness import brakedown as B  # noqa: E402  (default dimensions only)

CURVE, BITS = "bn254", 254


def random_elements(rng, count):
    """count residues below 2^253 < p: valid Montgomery representations of random field elements."""
    v = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << (BITS - 1 - 192)) - 1)
    v[:, 0] |= np.uint64(1)
    return v


def random_matrix(rng, n, m, d):
    """CSC arrays of an n x m matrix with d distinct random columns in every row."""
    if n < 4096 or m < 64:
        cols = np.stack([rng.choice(m, d, replace=False) for _ in range(n)])
    else:
        cols = rng.integers(0, m, size=(n, d))
        while True:
            s = np.sort(cols, axis=1)
            bad = np.nonzero((s[:, 1:] == s[:, :-1]).any(axis=1))[0]
            if not len(bad):
                break
            cols[bad] = rng.integers(0, m, size=(len(bad), d))
    rows = np.repeat(np.arange(n), d)
    order = np.argsort(cols.reshape(-1), kind="stable")
    ind_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols.reshape(-1), minlength=m))])
    return ind_ptr.astype(np.uintp), rows[order].astype(np.uint32)


def median_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def microbench_rate():
    exe = os.path.join(HERE, "microbench")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"fmul bn254_fr\s+\(8 limbs\)\s+[\d.]+ ms\s+([\d.]+) G mulmod/s", out)
    return float(m.group(1)) if m else None


def host_port_ms(nv, reps):
    exe = os.path.join(ROOT, "tests", "cpp", "brakedown_driver")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe, "time", str(nv), "16", str(reps)], capture_output=True, text=True, timeout=900).stdout
    m = re.search(r"host_encode_ms ([\d.]+)", out)
    return float(m.group(1)) if m else None


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [12, 14, 16, 18, 20, 22, 24]
    rate = microbench_rate()
    ctx = pc.Context(0)
    ctx.set_timing(True)
    rng = np.random.default_rng(0xB4A)
    rows_out = []
    for nv in sizes:
        n, m, a_dims, b_dims, m_ext = B.default_shape(1 << nv, BITS)
        mats = [random_matrix(rng, *d) for d in a_dims + b_dims]
        dims = [x for d in a_dims + b_dims for x in d]
        ind_ptr = np.concatenate([x[0] for x in mats])
        col_ind = np.concatenate([x[1] for x in mats])
        nnz = len(col_ind)
        code = ctx.brakedown_code(CURVE, m, m_ext, dims, ind_ptr, col_ind, random_elements(rng, nnz))
        mat = random_elements(rng, n * m).reshape(n, m, 4)
        x = torch.from_numpy(mat.view(np.int64)).cuda()
        y = torch.empty((n, m_ext, 4), dtype=torch.int64, device="cuda")
        ext = np.zeros((n, m_ext, 4), dtype=np.uint64)
        reps = 5 if nv >= 22 else 9
        enc = median_ms(lambda: code.encode(x, rows=n, out=y), 2, reps)
        phases = []
        for _ in range(reps):
            code.commit(x, rows=n, ext_out=y, want_leaves=False)
            phases.append(ctx.last_brakedown_phases_ms())
        ph = [statistics.median(p[i] for p in phases) for i in range(4)]
        dev_commit = median_ms(lambda: code.commit(x, rows=n, ext_out=y), 1, reps)
        host_commit = median_ms(lambda: code.commit(mat, ext_out=ext), 1, reps)
        code.free()
        host = host_port_ms(nv, 3)
        rec = dict(num_vars=nv, rows=n, m=m, m_ext=m_ext, nnz=nnz, encode_ms=enc[0], encode_min_max_ms=enc[1:], phases_ms=ph, commit_device_ms=dev_commit[0],
                   commit_host_ms=host_commit[0], host_port_16_threads_ms=host, speedup_vs_host_port=(host / enc[0]) if host else None,
                   gmul_per_s=n * nnz / enc[0] * 1e-6, fraction_of_fmul_rate=(n * nnz / enc[0] * 1e-6 / rate) if rate else None, fmul_bn254_fr_G_per_s=rate)
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)
    print("\n| num_vars | rows x m -> m_ext | non-zeros | encode ms (min-max) | A chain + base / B / digests / tree ms | commit dev ms | commit host ms | host port, 16 threads ms | x | G mul/s | of fmul rate |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows_out:
        f = lambda v, spec="%.3f": "-" if v is None else spec % v   # noqa: E731
        print(f"| {r['num_vars']} | {r['rows']} x {r['m']} -> {r['m_ext']} | {r['nnz']} | {r['encode_ms']:.3f} ({r['encode_min_max_ms'][0]:.3f}-{r['encode_min_max_ms'][1]:.3f}) | "
              + " / ".join("%.3f" % v for v in r["phases_ms"]) + f" | {r['commit_device_ms']:.3f} | {r['commit_host_ms']:.2f} | {f(r['host_port_16_threads_ms'], '%.1f')} | "
              f"{f(r['speedup_vs_host_port'], '%.0f')} | {r['gmul_per_s']:.1f} | {f(r['fraction_of_fmul_rate'])} |")
    ctx.close()


if __name__ == "__main__":
    main()
