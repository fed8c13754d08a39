// TEST-ONLY probe unit: the pieces of sample_generators on ed_on_bls12_381 (csrc/te_setup.hpp) one per lane -- the square root in Fq, the
// digest of a lane's message, from_random_bytes on given digests -- and the product's own per-index body, TeSampleBody, run as it is.
// For tests/test_te_setup_{cpu,gpu}.py (tests/harness/tesetupprobe.py).  The adapters only hand the bodies their pointers; the name is
// laid out on the host and passed by value, as abi_te_setup.hip does.
#include "probe_te_runner.hpp"
#include "../../poly_commit_amd/csrc/te_setup.hpp"

namespace probe_te_setup {
typedef pc_te_ed_on_bls12_381 T;
typedef pc::TeOf<T> TeC;
typedef pc::Fd<T::FqP> Fq;
constexpr size_t XW = pc::XyzzD<TeC>::WORDS, FN = Fq::N;

// in: v (Montgomery); out: root (Montgomery, zero for a non-square) | 1 if v is a square
struct SqrtBody {
  const uint32_t* in; uint32_t* out;
  PC_HD void operator()(uint32_t lane) const {
    Fq r = Fq::zero();
    const bool sq = pc::te_sqrt_ratio<T>(Fq::load(in + (size_t)lane * FN), Fq::one(), &r);
    uint32_t* o = out + (size_t)lane * (FN + 1);
    (sq ? r : Fq::zero()).store(o); o[FN] = sq ? 1u : 0u;
  }
};
// in: i lo | i hi | retry | j lo | j hi; out: the digest's 8 words
struct DigestBody {
  pc::TeSetupName name; const uint32_t* in; uint32_t* out;
  PC_HD void operator()(uint32_t lane) const {
    const uint32_t* p = in + (size_t)lane * 5;
    pc::te_setup_digest(name, (uint64_t)p[0] | ((uint64_t)p[1] << 32), p[2] != 0, (uint64_t)p[3] | ((uint64_t)p[4] << 32), out + (size_t)lane * 8);
  }
};
// in: a digest's 8 words; out: outcome (pc::TE_TRY_*) | x | y (Montgomery; zero unless accepted)
struct TryBody {
  const uint32_t* in; uint32_t* out;
  PC_HD void operator()(uint32_t lane) const {
    Fq x = Fq::zero(), y = Fq::zero();
    const uint32_t why = pc::te_from_random_bytes<T>(in + (size_t)lane * 8, &x, &y);
    uint32_t* o = out + (size_t)lane * (1 + 2 * FN);
    o[0] = why;
    if (why != pc::TE_TRY_ACCEPT) { x = Fq::zero(); y = Fq::zero(); }
    x.store(o + 1); y.store(o + 1 + FN);
  }
};
}  // namespace probe_te_setup
using namespace probe_te_setup;

extern "C" int pc_probe_te_setup_sqrt(size_t n, const uint32_t* in, uint32_t* out) {
  const probe::Buf bufs[] = {{in, nullptr, n * FN}, {nullptr, out, n * (FN + 1)}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return SqrtBody{d[0], d[1]}; });
}

extern "C" int pc_probe_te_setup_digest(const uint8_t* name, size_t name_len, size_t n, const uint32_t* in, uint32_t* out) {
  pc::TeSetupName nm;
  if (!nm.set(name, name_len)) return PROBE_BAD_OP;
  const probe::Buf bufs[] = {{in, nullptr, n * 5}, {nullptr, out, n * 8}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return DigestBody{nm, d[0], d[1]}; });
}

extern "C" int pc_probe_te_setup_try(size_t n, const uint32_t* in, uint32_t* out) {
  const probe::Buf bufs[] = {{in, nullptr, n * 8}, {nullptr, out, n * (1 + 2 * FN)}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return TryBody{d[0], d[1]}; });
}

// generators [first, first + n) times the cofactor: ext = n x 32 extended words, digests = n counts, failed = one word
extern "C" int pc_probe_te_setup_sample(const uint8_t* name, size_t name_len, uint64_t first, size_t n, uint32_t* ext, uint32_t* digests,
                                        uint32_t* failed) {
  pc::TeSetupName nm;
  if (!nm.set(name, name_len)) return PROBE_BAD_OP;
  const probe::Buf bufs[] = {{nullptr, ext, n * XW}, {nullptr, digests, n}, {nullptr, failed, 1}};
  return probe::run_bufs(n, bufs, 3, [&](uint32_t* const* d) {
    pc::TeSampleBody<TeC> b; b.name = nm; b.first = first; b.ext = d[0]; b.digests = d[1]; b.failed = d[2]; return b;
  });
}
