// TEST-ONLY probe unit: chains of mixed additions on the radix-2^30 running sum, one lane per index list (all lists in ONE launch)
#include "probe_runner.hpp"
#include "probe_bodies.hpp"

// in: lanes x (1 + max_steps) words; table: 64 affine points of 24 words; out: lanes x Chain30Body::OUT_WORDS
extern "C" int pc_probe_chain30(size_t lanes, uint32_t max_steps, const uint32_t* in, const uint32_t* table, uint32_t* out) {
  return probe::Runner::run<probe::Chain30Body>(lanes, in, lanes * (1 + (size_t)max_steps), out, lanes * probe::Chain30Body::OUT_WORDS, table, 64 * 24,
                                                max_steps);
}
