// Everything templated on the curve, instantiated for bls12_377 (see pc_internal.hpp).
#include "curve_ops_impl.hpp"
namespace pc {
const CurveOps& curve_ops_bls12_377() { static const CurveOps t = CurveOpsImpl<pc_curve_bls12_377>::table(); return t; }
}
