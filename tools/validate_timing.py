"""Time the validation of a resident key on the device (pc_hip_srs_check) and, in the same run, the host build of the same bodies on the
box's CPUs as the baseline.  Modelled on tools/sw_setup_timing.py.

Per curve in {bls12_381, bn254, pallas, bls12_377} (or `--curves=a,b`) and per count in {2^16, 2^20} (or the counts given), on a key made
by pc_hip_sample_generators (members of the subgroup: the ladders run to their end on every lane):
  - device: a blocking pc_hip_srs_check per pass -- the on-curve pass, the plain ladder by r (PC_HIP_SUBGROUP_LADDER=1; on BN254 and
    Pallas the ABI answers without a launch, so their ladder is timed through the probe on at most 2^16 points and marked so) and,
    on the two BLS12 curves, the fast test phi(P) = -[x^2] P (PC_HIP_SUBGROUP_LADDER=0): one warm-up, then 5 repeats, the median with
    minimum and maximum, points per second.
  - host: tests/hip/libpc_probe_host.so's pc_probe_validate_on_curve / _ladder / _fast (csrc/validate.hpp's bodies compiled by g++, the
    lanes looped over) on the last min(count, 2^16) points of the key -- at 2^16 the same points as the device -- (`--host-full`: the
    whole key at every count), split over 16 threads (ctypes releases the interpreter lock).  The last column is the ratio of the two
    RATES (points per second); the host's column says on how many points its rate was taken.
Every pass must report no failure, on the device and on the host.  The ratio "ladder / fast" of the device medians is what decides the
library's default between the two (abi_validate.hip, SubgroupFastDefault): DESIGN.md section 5 carries the figures.  Timing needs a GPU:
there is no fallback.  Prints one JSON line per measurement (profiles/validate_timing.jsonl is the record of a run) and a Markdown table."""
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
from harness import swvalidate as V  # noqa: E402

S = V.S
REPS = 5
HOST_THREADS = 16
HOST_COUNT = 1 << 16
PROBE_MAX = 1 << 16
PASSES = (("on_curve", "pc_probe_validate_on_curve"), ("ladder", "pc_probe_validate_ladder"), ("fast", "pc_probe_validate_fast"))


def host_pass(host, curve, entry, words):
    """the host build over the points on HOST_THREADS threads -> seconds"""
    cid = C.c_int(V.CURVE_ID[curve])
    step = (len(words) + HOST_THREADS - 1) // HOST_THREADS
    parts = [np.ascontiguousarray(words[s:s + step]) for s in range(0, len(words), step)]

    def one(w):
        flags = np.zeros(len(w), dtype=np.uint32)
        assert host.raw(entry, cid, C.c_size_t(len(w)), V.P().p32(w), V.P().p32(flags)) == 0
        return int(flags.sum())
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=HOST_THREADS) as ex:
        passed = sum(ex.map(one, parts))
    dt = time.perf_counter() - t0
    assert passed == len(words), "the host build rejects a generated point"
    return dt


def device_pass(key, name):
    os.environ["PC_HIP_SUBGROUP_LADDER"] = "1" if name == "ladder" else "0"
    times = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        got = key.check(on_curve=name == "on_curve", subgroup=name != "on_curve")
        dt = (time.perf_counter() - t0) * 1e3
        assert got == (0, None), "the device rejects a generated point"
        if rep:
            times.append(dt)
    return times


def probe_pass(dev, curve, entry, words):
    """a pass the ABI never launches (the ladder on a curve of cofactor 1), through the device probe: allocation and copies are in it"""
    times = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        flags = V.run_flags(dev, entry, (C.c_int(V.CURVE_ID[curve]),), words)
        dt = (time.perf_counter() - t0) * 1e3
        assert int(flags.sum()) == len(words)
        if rep:
            times.append(dt)
    return times


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    counts = [int(a) for a in args] or [1 << 16, 1 << 20]
    curves = list(V.CURVES)
    for a in sys.argv[1:]:
        if a.startswith("--curves="):
            curves = a.split("=", 1)[1].split(",")
    host_full = "--host-full" in sys.argv
    ctx = pc.Context(0)          # before the probe: the binding brings the runtime up first (poly_commit_amd/_ffi.py, load_library)
    host, dev = V.host_probe(), V.device_probe()
    rows = []
    for curve in curves:
        for count in counts:
            key = ctx.sample_generators(curve, S.IPA_NAME, 0, count)
            hcount = count if host_full else min(count, HOST_COUNT)
            tail = np.ascontiguousarray(key.read(count - hcount, hcount)).view(np.uint32)
            for name, entry in PASSES:
                if name == "fast" and curve not in V.BLS12:
                    continue
                via_probe = name == "ladder" and curve not in V.BLS12
                if via_probe:
                    pw = np.ascontiguousarray(key.read(0, min(count, PROBE_MAX))).view(np.uint32)
                    times, dcount = probe_pass(dev, curve, entry, pw), len(pw)
                else:
                    times, dcount = device_pass(key, name), count
                hsec = host_pass(host, curve, entry, tail)
                med = statistics.median(times)
                row = dict(curve=curve, count=count, what=name, via_probe=via_probe, device_count=dcount, device_ms=round(med, 3),
                           device_ms_min=round(min(times), 3), device_ms_max=round(max(times), 3), device_pts_per_s=round(dcount / med * 1e3),
                           host_threads=HOST_THREADS, host_count=hcount, host_ms=round(hsec * 1e3, 1), host_pts_per_s=round(hcount / hsec))
                row["rate_ratio"] = round(row["device_pts_per_s"] / row["host_pts_per_s"], 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
            key.free()
    ctx.close()
    os.environ.pop("PC_HIP_SUBGROUP_LADDER", None)
    print("\n| curve | points | pass | device ms (min .. max) | points/s | host (16 threads) points/s, on how many points | device rate / host rate |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %s%s | %.3f (%.3f .. %.3f) | %.3g | %.3g (%d points in %.0f ms) | %.1f |" % (
            r["curve"], r["count"], r["what"], " (probe, %d points, copies included)" % r["device_count"] if r["via_probe"] else "", r["device_ms"],
            r["device_ms_min"], r["device_ms_max"], r["device_pts_per_s"], r["host_pts_per_s"], r["host_count"], r["host_ms"], r["rate_ratio"]))
    for curve in curves:
        for count in counts:
            t = {r["what"]: r["device_ms"] for r in rows if r["curve"] == curve and r["count"] == count}
            if "fast" in t:
                print("%s, %d points: plain ladder / fast test = %.2f" % (curve, count, t["ladder"] / t["fast"]))


if __name__ == "__main__":
    main()
