"""Time InnerProductArgPC::setup's sample_generators over ed_on_bls12_381 on the device (pc_hip_te_sample_generators) and, in the same
run, the host build of the same per-index body on the box's CPUs as the baseline.

Per count in {2^16, 2^20 + 2} (or the counts given; 2^20 + 2 is setup at max_degree 2^20 - 1):
  - device: a blocking pc_hip_te_sample_generators with the reference's name, digest counts wanted: one warm-up (it grows the
    context's workspace), then 5 repeats; median with minimum and maximum, generators per second, and the mean and the maximum of
    out_digests_host -- a wave waits for the slowest of its 64 lanes, so the mean over the waves of the per-wave maximum is printed
    too: it is what the kernel pays per wave against the mean of 2.2 digests a lane would pay alone.
  - host: tests/hip/libpc_probe_host.so's pc_probe_te_setup_sample (csrc/te_setup.hpp's TeSampleBody compiled by g++, the lanes looped
    over; the batch normalisation is NOT in it: one inversion per 16 points on the device, a few percent), the index range split over
    16 threads (ctypes releases the interpreter lock).  The host runs 2^16 generators whatever the count is (`--host-full`: the whole
    count) and is compared in generators per second.
The first and last digest counts and the last point of the device run are compared with the host build's as a sanity check.  Timing
needs a GPU: there is no fallback.  Prints one JSON line per measurement and a Markdown table."""
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
from harness import tesetupprobe as P  # noqa: E402

TE = "ed_on_bls12_381"
NAME = b"PC-DL-2020"
REPS = 5
HOST_THREADS = 16
HOST_COUNT = 1 << 16


def host_sample(host, first, count):
    """the host build over [first, first + count) on HOST_THREADS threads -> (seconds, digest counts, extended words of the last index)"""
    step = (count + HOST_THREADS - 1) // HOST_THREADS
    parts = [(first + s, min(step, count - s)) for s in range(0, count, step)]

    def one(part):
        f, n = part
        ext, dg, failed = np.zeros((n, P.XW), dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        rc = host.raw("pc_probe_te_setup_sample", NAME, C.c_size_t(len(NAME)), C.c_uint64(f), C.c_size_t(n), P.T.p32(ext), P.T.p32(dg), P.T.p32(failed))
        assert rc == 0 and failed[0] == 0
        return dg, ext[-1]
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=HOST_THREADS) as ex:
        out = list(ex.map(one, parts))
    dt = time.perf_counter() - t0
    return dt, np.concatenate([d for d, _ in out]), out[-1][1]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    counts = [int(a) for a in args] or [1 << 16, (1 << 20) + 2]
    host_full = "--host-full" in sys.argv
    host = P.T.host_probe()
    ctx = pc.Context(0)
    rows = []
    for count in counts:
        times, digests, key = [], None, None
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            key, digests = ctx.te_sample_generators(TE, NAME, 0, count, want_digests=True)      # blocks: the counts are on the host
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                times.append(dt)
            if rep < REPS:
                key.free()
        last = key.read(count - 1, 1)[0]
        key.free()
        wave_max = [int(digests[s:s + 64].max()) for s in range(0, count, 64)]
        hcount = count if host_full else min(count, HOST_COUNT)
        hsec, hdig, hext = host_sample(host, count - hcount, hcount)
        assert (hdig == digests[count - hcount:]).all(), "device and host digest counts differ"
        X, Y, Z = (int.from_bytes(hext[8 * k:8 * k + 8].tobytes(), "little") for k in range(3))
        zi = pow(Z, -1, P.Q)
        want = b"".join((v * zi % P.Q * P.T.MONT % P.Q).to_bytes(32, "little") for v in (X, Y))      # the words are Montgomery: X / Z is not
        assert last.tobytes() == want, "device and host points differ"
        med = statistics.median(times)
        row = dict(count=count, device_ms=round(med, 3), device_ms_min=round(min(times), 3), device_ms_max=round(max(times), 3),
                   device_gen_per_s=round(count / med * 1e3), digests_mean=round(float(digests.mean()), 3), digests_max=int(digests.max()),
                   wave_max_mean=round(statistics.mean(wave_max), 3), host_threads=HOST_THREADS, host_count=hcount,
                   host_ms=round(hsec * 1e3, 1), host_gen_per_s=round(hcount / hsec))
        row["speedup"] = round(row["device_gen_per_s"] / row["host_gen_per_s"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    print("\n| generators | device ms (min .. max) | generators/s | digests mean / max | per-wave max, mean | host (16 threads) generators/s | ratio |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.3f (%.3f .. %.3f) | %.3g | %.3f / %d | %.2f | %.3g (%d generators in %.0f ms) | %.1f |" % (
            r["count"], r["device_ms"], r["device_ms_min"], r["device_ms_max"], r["device_gen_per_s"], r["digests_mean"], r["digests_max"],
            r["wave_max_mean"], r["host_gen_per_s"], r["host_count"], r["host_ms"], r["speedup"]))


if __name__ == "__main__":
    main()
