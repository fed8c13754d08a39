"""Child process of tests/test_sw_validate_gpu.py: pc_hip_srs_check over planted keys of the two BLS12 curves at every size of
harness.swvalidate.SIZES -- the keys of test_planted_non_members: a non-member at each edge index one at a time, then all at once, and,
from 65 points on, non-members beside records off the curve -- every window, with the subgroup bit alone and with both bits (the ladder
behind the on-curve gate), one JSON line per query.  The parent runs it once with PC_HIP_SUBGROUP_LADDER=0 and once with =1 (a fresh
process each) and compares the two outputs, and both with the reference."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import poly_commit_amd as pc  # noqa: E402
from harness import swvalidate as V  # noqa: E402


def keys(curve, n):
    """(name, kind, planted indices, start, windows or None) of the keys of one size; shared with the parent, which rebuilds the expectations"""
    at = V.plant_indices(n)
    out = [("one at %d" % i, "subgroup", [i], j + n, [(0, n), (i, 1), (0, i), (i + 1, n - i - 1)]) for j, i in enumerate(at)]
    out.append(("all at once", "subgroup", at, 0, None))
    if n >= 65:
        out.append(("beside off-curve records", "both", at, n, None))
    return out


def main():
    ctx = pc.Context(0)
    for curve in V.BLS12:
        for n in V.SIZES:
            for name, kind, at, start, wins in keys(curve, n):
                words, on, _ = V.planted_key(curve, n, at, kind=kind, start=start)
                key = V.upload_words(ctx, curve, words)
                for off, cnt in wins or V.windows(n, at):
                    for on_curve in (False, True):
                        if not on_curve and not all(on):
                            continue                   # the subgroup bit alone assumes on-curve points
                        bad, first, flags = key.check(off, cnt, on_curve=on_curve, subgroup=True, want_flags=True)
                        print(json.dumps(dict(curve=curve, n=n, key=name, offset=off, count=cnt, on_curve=on_curve, bad=bad, first=first,
                                              flags="".join(str(int(v)) for v in flags))))
                key.free()
    ctx.close()
    print("validate worker done, PC_HIP_SUBGROUP_LADDER=%s" % os.environ.get("PC_HIP_SUBGROUP_LADDER", ""))


if __name__ == "__main__":
    main()
