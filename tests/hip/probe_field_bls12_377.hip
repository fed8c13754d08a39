// TEST-ONLY probe unit: every Fd<P> operation of the two fields of BLS12-377 (which = 0: Fq, 1: Fr); op = probe::FieldOp.
// The unit names its set itself (probe_sets.hpp lists the sets of probe_field.hip, which compiles once per -DPROBE_SET).
#include "probe_runner.hpp"
#include "probe_bodies.hpp"
#define PROBE_ENTRY(stem) stem##_bls12_377
#define PROBE_FQ pc_bls12_377_fq
#define PROBE_FR pc_bls12_377_fr

extern "C" int PROBE_ENTRY(pc_probe_field)(int which, int op, size_t n, const uint32_t* in, uint32_t* out) {
  if (which == 0) return probe::dispatch<probe::FieldBodies<PROBE_FQ>::Body, probe::F_NOPS>(op, n, in, out);
  return probe::dispatch<probe::FieldBodies<PROBE_FR>::Body, probe::F_NOPS>(op, n, in, out);
}
// bit 0: LAZY_OK, bit 1: LAZY_FUSED_OK, as the code under test decides them (the tests derive them from the moduli)
extern "C" int PROBE_ENTRY(pc_probe_field_lazy)(int which) {
  if (which == 0) return (pc::Fd<PROBE_FQ>::LAZY_OK ? 1 : 0) | (pc::Fd<PROBE_FQ>::LAZY_FUSED_OK ? 2 : 0);
  return (pc::Fd<PROBE_FR>::LAZY_OK ? 1 : 0) | (pc::Fd<PROBE_FR>::LAZY_FUSED_OK ? 2 : 0);
}
extern "C" int PROBE_ENTRY(pc_probe_field_lazy_store)(int which) {
  return which == 0 ? (pc::Fd<PROBE_FQ>::LAZY_STORE_OK ? 1 : 0) : (pc::Fd<PROBE_FR>::LAZY_STORE_OK ? 1 : 0);
}
