// TEST-ONLY probe unit: the two-lane XYZZ addition of one G1 curve, n cases on 2 n pair lanes + n single lanes of one launch
#include "probe_runner.hpp"
#include "probe_halfadd.hpp"
#include "probe_sets.hpp"

extern "C" int PROBE_ENTRY(pc_probe_half_add)(size_t n, const uint32_t* in, uint32_t* out) {
  typedef probe::HalfAddBody<PROBE_CURVE> B;
  return probe::Runner::run<B>(3 * n, in, n * B::IN_WORDS, out, n * B::OUT_WORDS, nullptr, 0, (uint32_t)n);
}
