// TEST-ONLY probe unit: the key validation bodies of csrc/validate.hpp run as they are, one point per lane -- the on-curve test, the
// plain ladder by r (all four curves), the fast test of the two BLS12 curves, the two G2 bodies of BLS12-381 and the tally -- and the
// generated constants of the fast test.  For tests/test_sw_validate_{cpu,gpu}.py (tests/harness/swvalidate.py) and
// tools/validate_timing.py.  `curve` is a pc_curve id (0 .. 3); every entry returns PROBE_BAD_OP for an id it has no body for.  The
// adapters only hand the bodies their pointers; the NAF of r is made on the host and passed by value, as abi_validate.hip does.
#include "probe_te_runner.hpp"
#include "../../poly_commit_amd/csrc/validate.hpp"

namespace probe_validate {

template <class C> int on_curve_run(size_t n, const uint32_t* in, uint32_t* flags) {
  const probe::Buf bufs[] = {{in, nullptr, n * pc::AffD<C>::WORDS}, {nullptr, flags, n}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return pc::SwOnCurveBody<C>{d[0], d[1]}; });
}
// G: a curve, or pc::G2Of<curve>
template <class G> int ladder_run(size_t n, const uint32_t* in, uint32_t* flags) {
  const probe::Buf bufs[] = {{in, nullptr, n * pc::AffD<G>::WORDS}, {nullptr, flags, n}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) {
    pc::SwSubgroupLadderBody<G> b; b.key = d[0]; b.flags = d[1]; b.gate = nullptr; b.set_order(); return b;
  });
}
template <class C> int fast_run(size_t n, const uint32_t* in, uint32_t* flags) {
  const probe::Buf bufs[] = {{in, nullptr, n * pc::AffD<C>::WORDS}, {nullptr, flags, n}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return pc::Bls12SubgroupBody<C>{d[0], d[1], nullptr}; });
}
template <class C> int constants(uint32_t* out) {
  typedef pc_subgroup_constants<C> K;
  out[0] = (uint32_t)K::X_ABS; out[1] = (uint32_t)(K::X_ABS >> 32); out[2] = (uint32_t)K::X_NEG; out[3] = (uint32_t)K::BETA_IS_GLV;
  for (int i = 0; i < C::FqP::N; i++) out[4 + i] = K::BETA_MONT[i];
  return 0;
}

}  // namespace probe_validate
using namespace probe_validate;

#define PROBE_VALIDATE_DISPATCH(curve, fn, ...)                            \
  switch (curve) {                                                         \
    case 0: return fn<pc_curve_bls12_381>(__VA_ARGS__);                    \
    case 1: return fn<pc_curve_bn254>(__VA_ARGS__);                        \
    case 2: return fn<pc_curve_pallas>(__VA_ARGS__);                       \
    case 3: return fn<pc_curve_bls12_377>(__VA_ARGS__);                    \
  }                                                                        \
  return PROBE_BAD_OP
#define PROBE_VALIDATE_BLS12(curve, fn, ...)                               \
  switch (curve) {                                                         \
    case 0: return fn<pc_curve_bls12_381>(__VA_ARGS__);                    \
    case 3: return fn<pc_curve_bls12_377>(__VA_ARGS__);                    \
  }                                                                        \
  return PROBE_BAD_OP

// in: n affine points x || y as a resident key holds them (raw words: they need not be residues); flags: n words
extern "C" int pc_probe_validate_on_curve(int curve, size_t n, const uint32_t* in, uint32_t* flags) { PROBE_VALIDATE_DISPATCH(curve, on_curve_run, n, in, flags); }
extern "C" int pc_probe_validate_ladder(int curve, size_t n, const uint32_t* in, uint32_t* flags) { PROBE_VALIDATE_DISPATCH(curve, ladder_run, n, in, flags); }
extern "C" int pc_probe_validate_fast(int curve, size_t n, const uint32_t* in, uint32_t* flags) { PROBE_VALIDATE_BLS12(curve, fast_run, n, in, flags); }
// out: |x| low, |x| high, 1 if x < 0, 1 if beta' is the GLV header's BETA, then beta' (Montgomery, 12 words)
extern "C" int pc_probe_validate_constants(int curve, uint32_t* out) { PROBE_VALIDATE_BLS12(curve, constants, out); }
// BLS12-381 G2, points x.c0 || x.c1 || y.c0 || y.c1; op 0: G2OnCurveBody, 1: G2SubgroupBody
extern "C" int pc_probe_validate_g2(int op, size_t n, const uint32_t* in, uint32_t* flags) {
  typedef pc_curve_bls12_381 C;
  if (op == 1) return ladder_run<pc::G2Of<C>>(n, in, flags);
  if (op != 0) return PROBE_BAD_OP;
  const probe::Buf bufs[] = {{in, nullptr, n * pc::AffD<pc::G2Of<C>>::WORDS}, {nullptr, flags, n}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return pc::G2OnCurveBody<C>{d[0], d[1]}; });
}
// ValidateTallyBody over n flags: ok = n bytes in ceil(n / 4) words, out = failures | lowest failing index (0xffffffff: none)
extern "C" int pc_probe_validate_tally(size_t n, const uint32_t* flags, uint32_t* ok_words, uint32_t* out) {
  const uint32_t init[2] = {0u, 0xffffffffu};
  const probe::Buf bufs[] = {{flags, nullptr, n}, {nullptr, ok_words, (n + 3) / 4}, {init, out, 2}};
  return probe::run_bufs(n, bufs, 3, [&](uint32_t* const* d) { return pc::ValidateTallyBody{d[0], (uint8_t*)d[1], d[2], d[2] + 1}; });
}
