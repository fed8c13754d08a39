// The curve ids of include/pc_hip.h as the ABI units check them: one bound for every entry point, and the one size that
// depends on the id alone.  (Host only, no templates: group.hip includes it without the kernels.)
#pragma once
#include <stddef.h>
#include "../../include/pc_hip.h"

constexpr int PC_CURVE_LAST = PC_CURVE_BLS12_377;      // the highest id with a CurveOps / FieldOps table (pc_internal.hpp)

inline bool pc_known_curve(pc_curve c) { return (int)c >= 0 && (int)c <= PC_CURVE_LAST; }
// bytes of one base-field element: 12 words for the two BLS12 curves, 8 for BN254 and Pallas
inline size_t pc_fq_bytes(pc_curve c) { return c == PC_CURVE_BLS12_381 || c == PC_CURVE_BLS12_377 ? 48 : 32; }
