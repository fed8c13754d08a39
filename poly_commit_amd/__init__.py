"""MI355X (gfx950) backend for the commit/open hot path of arkworks-rs/poly-commit.

Python is only the harness language here (tests, bench, torch.distributed plumbing); the
product is the C-ABI library ``libpc_hip.so`` (include/pc_hip.h) built from ``csrc/``.
"""
from ._ffi import (  # noqa: F401
    CHECK_ON_CURVE, CHECK_SUBGROUP, CURVES, TE_CURVES, BrakedownCode, Context, G2Srs, Group, GroupSrs, PcHipError, Srs, TeSrs, g2_point_mul, g2_points_sum, library_path, load_library, ml_level_offset, multilinear_pair_key,
    point_mul, points_sum, te_point_mul, te_points_sum, universal_params_layout,
)
