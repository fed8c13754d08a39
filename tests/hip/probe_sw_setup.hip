// TEST-ONLY probe unit: the pieces of sample_generators on the short Weierstrass curves (csrc/sw_setup.hpp) one operand per lane -- the
// square root in the base field, from_random_bytes on caller-supplied digests, the cofactor multiplication -- and the product's own
// per-index body, SwSampleBody, run as it is.  For tests/test_sw_setup_cpu.py, tests/test_sw_primitives_gpu.py and
// tools/sw_setup_timing.py.  `curve` is a pc_curve id (0 .. 3); every entry returns PROBE_BAD_OP for another one.  The adapters only
// hand the bodies their pointers; the name is laid out on the host and passed by value, as abi_setup.hip does.
#include "probe_te_runner.hpp"
#include "../../poly_commit_amd/csrc/sw_setup.hpp"

namespace probe_sw_setup {

// in: v (Montgomery); out: root (Montgomery, zero for a non-square) | 1 if v is a square
template <class C>
struct SqrtBody {
  typedef pc::Fd<typename C::FqP> Fq;
  const uint32_t* in; uint32_t* out;
  PC_HD void operator()(uint32_t lane) const {
    Fq r = Fq::zero();
    const bool sq = pc::sw_sqrt<typename C::FqP>(Fq::load(in + (size_t)lane * Fq::N), &r);
    uint32_t* o = out + (size_t)lane * (Fq::N + 1);
    (sq ? r : Fq::zero()).store(o); o[Fq::N] = sq ? 1u : 0u;
  }
};
// in: a digest's 8 words; out: outcome (pc::SW_TRY_*) | x | y (Montgomery; zero unless accepted)
template <class C>
struct TryBody {
  typedef pc::Fd<typename C::FqP> Fq;
  const uint32_t* in; uint32_t* out;
  PC_HD void operator()(uint32_t lane) const {
    Fq x = Fq::zero(), y = Fq::zero();
    const uint32_t why = pc::sw_from_random_bytes<C>(in + (size_t)lane * 8, &x, &y);
    uint32_t* o = out + (size_t)lane * (1 + 2 * Fq::N);
    o[0] = why;
    if (why != pc::SW_TRY_ACCEPT) { x = Fq::zero(); y = Fq::zero(); }
    x.store(o + 1); y.store(o + 1 + Fq::N);
  }
};
// in: an affine point x || y (Montgomery, all zero: infinity); out: cofactor * point in XYZZ
template <class C>
struct CofactorBody {
  const uint32_t* in; uint32_t* out;
  PC_HD void operator()(uint32_t lane) const {
    pc::sw_mul_by_cofactor<C>(pc::AffD<C>::load(in + (size_t)lane * pc::AffD<C>::WORDS)).store(out + (size_t)lane * pc::XyzzD<C>::WORDS);
  }
};

template <class C> int sqrt_run(size_t n, const uint32_t* in, uint32_t* out) {
  constexpr size_t FN = C::FqP::N;
  const probe::Buf bufs[] = {{in, nullptr, n * FN}, {nullptr, out, n * (FN + 1)}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return SqrtBody<C>{d[0], d[1]}; });
}
template <class C> int try_run(size_t n, const uint32_t* in, uint32_t* out) {
  constexpr size_t FN = C::FqP::N;
  const probe::Buf bufs[] = {{in, nullptr, n * 8}, {nullptr, out, n * (1 + 2 * FN)}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return TryBody<C>{d[0], d[1]}; });
}
template <class C> int cofactor_run(size_t n, const uint32_t* in, uint32_t* out) {
  const probe::Buf bufs[] = {{in, nullptr, n * pc::AffD<C>::WORDS}, {nullptr, out, n * pc::XyzzD<C>::WORDS}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return CofactorBody<C>{d[0], d[1]}; });
}
template <class C> int sample_run(const pc::TeSetupName& nm, uint64_t first, size_t n, uint32_t* out, uint32_t* digests, uint32_t* failed) {
  const probe::Buf bufs[] = {{nullptr, out, n * pc::AffD<C>::WORDS}, {nullptr, digests, n}, {nullptr, failed, 1}};
  return probe::run_bufs(n, bufs, 3, [&](uint32_t* const* d) {
    pc::SwSampleBody<C> b; b.name = nm; b.first = first; b.out = d[0]; b.digests = d[1]; b.failed = d[2]; return b;
  });
}

}  // namespace probe_sw_setup
using namespace probe_sw_setup;

#define PROBE_SW_DISPATCH(curve, fn, ...)                                  \
  switch (curve) {                                                         \
    case 0: return fn<pc_curve_bls12_381>(__VA_ARGS__);                    \
    case 1: return fn<pc_curve_bn254>(__VA_ARGS__);                        \
    case 2: return fn<pc_curve_pallas>(__VA_ARGS__);                       \
    case 3: return fn<pc_curve_bls12_377>(__VA_ARGS__);                    \
  }                                                                        \
  return PROBE_BAD_OP

extern "C" int pc_probe_sw_setup_sqrt(int curve, size_t n, const uint32_t* in, uint32_t* out) { PROBE_SW_DISPATCH(curve, sqrt_run, n, in, out); }
extern "C" int pc_probe_sw_setup_try(int curve, size_t n, const uint32_t* in, uint32_t* out) { PROBE_SW_DISPATCH(curve, try_run, n, in, out); }
extern "C" int pc_probe_sw_setup_cofactor(int curve, size_t n, const uint32_t* in, uint32_t* out) { PROBE_SW_DISPATCH(curve, cofactor_run, n, in, out); }

// generators [first, first + n) BEFORE the cofactor (SwSampleBody): out = n affine points, digests = n counts, failed = one word
extern "C" int pc_probe_sw_setup_sample(int curve, const uint8_t* name, size_t name_len, uint64_t first, size_t n, uint32_t* out,
                                        uint32_t* digests, uint32_t* failed) {
  pc::TeSetupName nm;
  if (!nm.set(name, name_len)) return PROBE_BAD_OP;
  PROBE_SW_DISPATCH(curve, sample_run, nm, first, n, out, digests, failed);
}
