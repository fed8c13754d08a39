// TEST-ONLY probe unit: every Fd<P> operation of one curve's two fields (which = 0: Fq, 1: Fr); op = probe::FieldOp
#include "probe_runner.hpp"
#include "probe_bodies.hpp"
#include "probe_sets.hpp"

extern "C" int PROBE_ENTRY(pc_probe_field)(int which, int op, size_t n, const uint32_t* in, uint32_t* out) {
  if (which == 0) return probe::dispatch<probe::FieldBodies<PROBE_FQ>::Body, probe::F_NOPS>(op, n, in, out);
  return probe::dispatch<probe::FieldBodies<PROBE_FR>::Body, probe::F_NOPS>(op, n, in, out);
}
// bit 0: LAZY_OK, bit 1: LAZY_FUSED_OK, as the code under test decides them (the tests derive them from the moduli)
extern "C" int PROBE_ENTRY(pc_probe_field_lazy)(int which) {
  if (which == 0) return (pc::Fd<PROBE_FQ>::LAZY_OK ? 1 : 0) | (pc::Fd<PROBE_FQ>::LAZY_FUSED_OK ? 2 : 0);
  return (pc::Fd<PROBE_FR>::LAZY_OK ? 1 : 0) | (pc::Fd<PROBE_FR>::LAZY_FUSED_OK ? 2 : 0);
}
