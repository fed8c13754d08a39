// TEST-ONLY probe unit: the radix-2^30 field (op = probe::Fq30Op) and Fq2 of BLS12-381 (op = probe::Fq2Op)
#include "probe_runner.hpp"
#include "probe_bodies.hpp"

extern "C" int pc_probe_fq30(int op, size_t n, const uint32_t* in, uint32_t* out) { return probe::dispatch<probe::Fq30Body, probe::Q_NOPS>(op, n, in, out); }
extern "C" int pc_probe_fq2(int op, size_t n, const uint32_t* in, uint32_t* out) { return probe::dispatch<probe::Fq2Body, probe::E_NOPS>(op, n, in, out); }
