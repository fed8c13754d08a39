"""Time sample_generators over the short Weierstrass curves on the device (pc_hip_sample_generators) and, in the same run, the host
build of the same per-index bodies on the box's CPUs as the baseline.  Modelled on tools/te_setup_timing.py.

Per curve in {bls12_381, bn254, pallas, bls12_377} (or `--curves a,b`) and per count in {2^16, 2^20} (or the counts given):
  - device: a blocking pc_hip_sample_generators with the reference's name "PC-DL-2020", digest counts wanted: one warm-up (it grows the
    context's workspace), then 5 repeats; median with minimum and maximum, generators per second, and the mean and the maximum of
    out_digests_host -- a wave waits for the slowest of its 64 lanes, so the mean over the waves of the per-wave maximum is printed too.
  - host: tests/hip/libpc_probe_host.so's pc_probe_sw_setup_sample (csrc/sw_setup.hpp's SwSampleBody compiled by g++, the lanes looped
    over) followed, where the cofactor is not 1, by pc_probe_sw_setup_cofactor on its points (SwCofactorBody's work; the batch
    normalisation is NOT in it: one inversion per 16 points on the device), the index range split over 16 threads (ctypes releases the
    interpreter lock).  The host runs 2^14 generators whatever the count is (`--host-full`: the whole count) and is compared in
    generators per second.
The digest counts of the device run are compared with the host build's, and the last point with the host's (normalised here with
Python integers), as a sanity check.  Timing needs a GPU: there is no fallback.  Prints one JSON line per measurement and a Markdown
table."""
import concurrent.futures
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import poly_commit_amd as pc  # noqa: E402
from harness import sw_setup as S  # noqa: E402
from harness import swsetupprobe as P  # noqa: E402

NAME = S.IPA_NAME
REPS = 5
HOST_THREADS = 16
HOST_COUNT = 1 << 14


def host_sample(host, curve, first, count):
    """the host build over [first, first + count) on HOST_THREADS threads -> (seconds, digest counts, the last generator as a point)"""
    n = S.field(curve)[2]
    cid = C.c_int(S.CURVE_ID[curve])
    with_cofactor = S.cofactor(curve) != 1
    step = (count + HOST_THREADS - 1) // HOST_THREADS
    parts = [(first + s, min(step, count - s)) for s in range(0, count, step)]
    p32 = P.P().p32

    def one(part):
        f, k = part
        aff, dg, failed = np.zeros((k, 2 * n), dtype=np.uint32), np.zeros(k, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        rc = host.raw("pc_probe_sw_setup_sample", cid, NAME, C.c_size_t(len(NAME)), C.c_uint64(f), C.c_size_t(k), p32(aff), p32(dg), p32(failed))
        assert rc == 0 and failed[0] == 0
        ext = None
        if with_cofactor:
            ext = np.zeros((k, 4 * n), dtype=np.uint32)
            assert host.raw("pc_probe_sw_setup_cofactor", cid, C.c_size_t(k), p32(aff), p32(ext)) == 0
        return dg, aff[-1], None if ext is None else ext[-1]
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=HOST_THREADS) as ex:
        out = list(ex.map(one, parts))
    dt = time.perf_counter() - t0
    _, aff, ext = out[-1]
    if ext is None:
        last = S.point_of_words(curve, aff)
    else:
        prime = S.field(curve)[0]
        X, Y, ZZ, ZZZ = P.from_mont(curve, ext.reshape(4, n))
        last = (X * pow(ZZ, -1, prime) % prime, Y * pow(ZZZ, -1, prime) % prime)
    return dt, np.concatenate([d for d, _, _ in out]), last


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    counts = [int(a) for a in args] or [1 << 16, 1 << 20]
    curves = list(S.CURVES)
    for a in sys.argv[1:]:
        if a.startswith("--curves="):
            curves = a.split("=", 1)[1].split(",")
    host_full = "--host-full" in sys.argv
    host = P.host_probe()
    ctx = pc.Context(0)
    rows = []
    for curve in curves:
        for count in counts:
            times, digests, key = [], None, None
            for rep in range(REPS + 1):
                t0 = time.perf_counter()
                key, digests = ctx.sample_generators(curve, NAME, 0, count, want_digests=True)      # blocks: the counts are on the host
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    times.append(dt)
                if rep < REPS:
                    key.free()
            last = S.point_of_words(curve, np.ascontiguousarray(key.read(count - 1, 1)).view(np.uint32)[0])
            key.free()
            wave_max = [int(digests[s:s + 64].max()) for s in range(0, count, 64)]
            hcount = count if host_full else min(count, HOST_COUNT)
            hsec, hdig, hlast = host_sample(host, curve, count - hcount, hcount)
            assert (hdig == digests[count - hcount:]).all(), "device and host digest counts differ"
            assert last == hlast, "device and host points differ"
            med = statistics.median(times)
            row = dict(curve=curve, count=count, device_ms=round(med, 3), device_ms_min=round(min(times), 3), device_ms_max=round(max(times), 3),
                       device_gen_per_s=round(count / med * 1e3), digests_mean=round(float(digests.mean()), 3), digests_max=int(digests.max()),
                       wave_max_mean=round(statistics.mean(wave_max), 3), host_threads=HOST_THREADS, host_count=hcount,
                       host_ms=round(hsec * 1e3, 1), host_gen_per_s=round(hcount / hsec))
            row["speedup"] = round(row["device_gen_per_s"] / row["host_gen_per_s"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    print("\n| curve | generators | device ms (min .. max) | generators/s | digests mean / max | per-wave max, mean | host (16 threads) generators/s | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %.3f (%.3f .. %.3f) | %.3g | %.3f / %d | %.2f | %.3g (%d generators in %.0f ms) | %.1f |" % (
            r["curve"], r["count"], r["device_ms"], r["device_ms_min"], r["device_ms_max"], r["device_gen_per_s"], r["digests_mean"], r["digests_max"],
            r["wave_max_mean"], r["host_gen_per_s"], r["host_count"], r["host_ms"], r["speedup"]))


if __name__ == "__main__":
    main()
