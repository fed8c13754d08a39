// TEST-ONLY probe unit: the XYZZ group law of G1 of BLS12-377 (op = probe::CurveOp); the unit names its set itself (see
// probe_field_bls12_377.hip)
#include "probe_runner.hpp"
#include "probe_bodies.hpp"
#define PROBE_ENTRY(stem) stem##_bls12_377
#define PROBE_CURVE pc_curve_bls12_377

extern "C" int PROBE_ENTRY(pc_probe_curve)(int op, size_t n, const uint32_t* in, uint32_t* out) {
  return probe::dispatch<probe::CurveBodies<PROBE_CURVE>::Body, probe::C_NOPS>(op, n, in, out);
}
