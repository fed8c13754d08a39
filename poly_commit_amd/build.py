"""Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU).

The library is split into translation units that compile in parallel (one per curve, one per
scalar field, the ABI glue, the hash-only kernels); objects are cached under csrc/_obj and
rebuilt when any source or header is newer.

A second target, tests/hip/libpc_probe.so, is test infrastructure: the field and curve primitives of csrc/ one
per lane (tests/hip/probe_bodies.hpp, probe_te_bodies.hpp), for tests/test_device_primitives_gpu.py and its siblings, and two stages of
the MSM on their own: the bucket sort (probe_sort.hip) and the bucket reduction, level by level (probe_reduce.hip); probe_validate.hip runs the key
validation bodies (csrc/validate.hpp).  It has its own object cache
(tests/hip/_obj) and staleness check (its sources and the csrc headers); the product library does not contain it."""
import concurrent.futures
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["abi_ctx.hip", "abi_srs.hip", "abi_msm.hip", "abi_poly.hip", "abi_ipa.hip", "abi_lincode.hip", "abi_g2.hip", "abi_te.hip", "abi_te_ipa.hip", "abi_te_setup.hip", "abi_setup.hip", "abi_skzg.hip", "abi_pst13.hip", "abi_validate.hip", "group.hip", "hash_tu.hip",
           "curve_bls12_381.hip", "curve_bn254.hip", "curve_pallas.hip", "curve_bls12_377.hip",
           "field_bls12_381.hip", "field_bn254.hip", "field_pallas.hip", "field_bls12_377.hip"]
# PC_HIP_VARIANT=name builds an alternative library libpc_hip_<name>.so (own object cache) from the same sources with
# PC_HIP_CXXFLAGS -- kernel tuning experiments; load it with PC_HIP_LIB=<path>
_VARIANT = os.environ.get("PC_HIP_VARIANT", "")
OBJ = os.path.join(CSRC, "_obj" + ("_" + _VARIANT if _VARIANT else ""))
OUT = os.path.join(HERE, "libpc_hip" + ("_" + _VARIANT if _VARIANT else "") + ".so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"]
MAX_JOBS = 16

# the probe: (source, PROBE_SET or None); a unit with a set compiles once per curve (tests/hip/probe_sets.hpp), the others name
# their types themselves
PROBE_DIR = os.path.join(os.path.dirname(HERE), "tests", "hip")
PROBE_OBJ = os.path.join(PROBE_DIR, "_obj")
PROBE_OUT = os.path.join(PROBE_DIR, "libpc_probe.so")
PROBE_UNITS = ([("probe_field.hip", k) for k in range(3)] + [("probe_curve.hip", k) for k in range(4)] +
               [("probe_halfadd.hip", k) for k in range(3)] + [("probe_fq30.hip", None), ("probe_chain30.hip", None)] +
               [("probe_field_bls12_377.hip", None), ("probe_curve_bls12_377.hip", None)] +
               [("probe_field_te.hip", None), ("probe_te.hip", None), ("probe_te_setup.hip", None), ("probe_sw_setup.hip", None)] +
               [("probe_sort.hip", None), ("probe_reduce.hip", None), ("probe_validate.hip", None)])
# a unit whose source this tree's tests/hip does not have is left out: a tests/ tree from before the unit was added still builds its
# probe, and a test that needs the unit fails at its missing entry point
PROBE_UNITS = [u for u in PROBE_UNITS if os.path.exists(os.path.join(PROBE_DIR, u[0]))]


def _newest_header():
    t = os.path.getmtime(os.path.join(os.path.dirname(HERE), "include", "pc_hip.h"))
    for f in os.listdir(CSRC):
        if f.endswith((".hpp", ".h")):
            t = max(t, os.path.getmtime(os.path.join(CSRC, f)))
    return t


def _stale_objects():
    th = _newest_header()
    flags_tag = " ".join(FLAGS + os.environ.get("PC_HIP_CXXFLAGS", "").split())
    tag_file = os.path.join(OBJ, "flags.txt")
    same_flags = os.path.exists(tag_file) and open(tag_file).read() == flags_tag
    stale = []
    for s in SOURCES:
        o = os.path.join(OBJ, s.replace(".hip", ".o"))
        src_t = max(th, os.path.getmtime(os.path.join(CSRC, s)))
        if not same_flags or not os.path.exists(o) or os.path.getmtime(o) < src_t:
            stale.append(s)
    return stale, flags_tag


def needs_build():
    if not os.path.exists(OUT):
        return True
    stale, _ = _stale_objects()
    if stale:
        return True
    return any(os.path.getmtime(os.path.join(OBJ, s.replace(".hip", ".o"))) > os.path.getmtime(OUT) for s in SOURCES)


def _jobs(n):
    return max(1, min(n, MAX_JOBS, os.cpu_count() or 1))


def probe_object(unit):
    src, k = unit
    return os.path.join(PROBE_OBJ, src.replace(".hip", "") + ("" if k is None else "_%d" % k) + ".o")


def probe_sources():
    return sorted(os.path.join(PROBE_DIR, f) for f in os.listdir(PROBE_DIR) if f.endswith((".hip", ".hpp")))


def _probe_stale_units():
    src_t = max([_newest_header()] + [os.path.getmtime(f) for f in probe_sources()])
    return [u for u in PROBE_UNITS if not os.path.exists(probe_object(u)) or os.path.getmtime(probe_object(u)) < src_t]


def probe_needs_build():
    if not os.path.exists(PROBE_OUT) or _probe_stale_units():
        return True
    return any(os.path.getmtime(probe_object(u)) > os.path.getmtime(PROBE_OUT) for u in PROBE_UNITS)


def build_probe(force=False, verbose=False):
    """tests/hip/libpc_probe.so for gfx950 (skipped for a PC_HIP_VARIANT build and where the tree has no tests/hip)"""
    if _VARIANT or not os.path.isdir(PROBE_DIR):
        return None
    if not force and not probe_needs_build():
        return PROBE_OUT
    os.makedirs(PROBE_OBJ, exist_ok=True)
    stale = list(PROBE_UNITS) if force else _probe_stale_units()

    def compile_one(unit):
        src, k = unit
        cmd = ["hipcc"] + FLAGS + ([] if k is None else ["-DPROBE_SET=%d" % k]) + ["-c", os.path.join(PROBE_DIR, src), "-o", probe_object(unit)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with concurrent.futures.ThreadPoolExecutor(max_workers=_jobs(len(stale))) as ex:
        list(ex.map(compile_one, stale))
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", PROBE_OUT] + [probe_object(u) for u in PROBE_UNITS]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return PROBE_OUT


def build(force=False, verbose=False):
    """both targets; returns the path of the product library"""
    out = build_product(force, verbose)
    build_probe(force, verbose)
    return out


def build_product(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    os.makedirs(OBJ, exist_ok=True)
    stale, flags_tag = _stale_objects()
    if force:
        stale = list(SOURCES)
    extra = os.environ.get("PC_HIP_CXXFLAGS", "").split()

    def compile_one(s):
        o = os.path.join(OBJ, s.replace(".hip", ".o"))
        cmd = ["hipcc"] + FLAGS + extra + ["-c", os.path.join(CSRC, s), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return o

    with concurrent.futures.ThreadPoolExecutor(max_workers=_jobs(len(stale))) as ex:
        list(ex.map(compile_one, stale))
    with open(os.path.join(OBJ, "flags.txt"), "w") as f:
        f.write(flags_tag)
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    import sys
    build(force="--force" in sys.argv, verbose=True)
