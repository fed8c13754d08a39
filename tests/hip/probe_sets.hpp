// TEST-ONLY: the units of the probe compile once per curve (-DPROBE_SET=0..3) so that they build in parallel
#pragma once
#ifndef PROBE_SET
#error "compile with -DPROBE_SET=0 (BLS12-381), 1 (BN254), 2 (Pallas) or 3 (G2 of BLS12-381)"
#endif
#if PROBE_SET == 0
#define PROBE_ENTRY(stem) stem##_bls12_381
#define PROBE_FQ pc_bls12_381_fq
#define PROBE_FR pc_bls12_381_fr
#define PROBE_CURVE pc_curve_bls12_381
#elif PROBE_SET == 1
#define PROBE_ENTRY(stem) stem##_bn254
#define PROBE_FQ pc_bn254_fq
#define PROBE_FR pc_bn254_fr
#define PROBE_CURVE pc_curve_bn254
#elif PROBE_SET == 2
#define PROBE_ENTRY(stem) stem##_pallas
#define PROBE_FQ pc_pallas_fq
#define PROBE_FR pc_pallas_fr
#define PROBE_CURVE pc_curve_pallas
#else
#define PROBE_ENTRY(stem) stem##_bls12_381_g2
#define PROBE_CURVE pc::G2Of<pc_curve_bls12_381>
#endif
