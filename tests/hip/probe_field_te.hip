// TEST-ONLY probe unit: every Fd<P> operation of the two fields of ed_on_bls12_381 (which = 0: the coordinate field, BLS12-381's Fr,
// where LAZY_OK is false and the lazy operations are PROBE_UNSUPPORTED; 1: the curve's own scalar field of 252 bits, lazy throughout);
// op = probe::FieldOp.  The unit names its types itself, as probe_field_bls12_377.hip does.
#include "probe_runner.hpp"
#include "probe_bodies.hpp"
#include "../../poly_commit_amd/csrc/te_constants.h"
#define PROBE_ENTRY(stem) stem##_ed_on_bls12_381
#define PROBE_FQ pc_te_ed_on_bls12_381::FqP
#define PROBE_FR pc_te_ed_on_bls12_381::FrP

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
