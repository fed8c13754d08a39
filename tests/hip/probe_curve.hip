// TEST-ONLY probe unit: the XYZZ group law of one group (op = probe::CurveOp)
#include "probe_runner.hpp"
#include "probe_bodies.hpp"
#include "probe_sets.hpp"

extern "C" int PROBE_ENTRY(pc_probe_curve)(int op, size_t n, const uint32_t* in, uint32_t* out) {
  return probe::dispatch<probe::CurveBodies<PROBE_CURVE>::Body, probe::C_NOPS>(op, n, in, out);
}
