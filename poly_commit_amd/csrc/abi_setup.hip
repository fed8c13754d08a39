// C ABI of the gfx950 backend (include/pc_hip.h): InnerProductArgPC::setup / trim and HyraxPC::setup over the short Weierstrass curves
// of pc_curve on the device -- sample_generators (ipa_pc/mod.rs:302-325, hyrax/mod.rs:119-168) as a new resident pc_srs, and trim's
// prefix of a key (ipa_pc/mod.rs:384).  The kernels are sw_setup.hpp's (digest, from_random_bytes with its square root, the cofactor:
// one lane per index) and ipa.hpp's batch normalisation; the key object is key.hpp's.  This unit instantiates SwSampleBody for the four
// curves itself: nothing else in the library needs it.
#include "abi.hpp"
#include "ipa.hpp"
#include "sw_setup.hpp"

namespace pc {
namespace {

constexpr uint32_t SW_NORM_K = 16;      // points per inversion of the normalisation (TE_NORM_K's value)

// generators [first, first + count) of `name` into the resident points at dst; the digest counts to digests_host (or null).  Returns
// true if a lane hit the cap.  Drains the context's queue.
template <class C>
bool sample_run(HipBackend& be, const TeSetupName& name, uint64_t first, size_t count, uint32_t* dst, uint32_t* digests_host) {
  typedef SwSampleBody<C> Body;
  constexpr size_t AW = AffD<C>::WORDS, XW = XyzzD<C>::WORDS, FN = C::FqP::N;
  // (cofactor > 1) the points in XYZZ | the prefix products of the normalisation | the digest counts | the flag of the cap
  const size_t ext_words = Body::COFACTOR_ONE ? 0 : count * (XW + FN);
  uint32_t* ws = (uint32_t*)be.workspace((ext_words + count + 1) * 4);
  uint32_t* ext = ws;
  uint32_t* digests = ws + ext_words;
  uint32_t* failed = digests + count;
  be.memset(failed, 0, 4);
  // the points before the cofactor go to the key's own buffer: with cofactor 1 they are the key, otherwise the normalisation
  // overwrites them (it reads the XYZZ copies only)
  Body body;
  body.name = name; body.first = first; body.out = dst; body.digests = digests; body.failed = failed;
  be.launch(body, count);
  if constexpr (!Body::COFACTOR_ONE) {
    static_assert(AW * 2 == XW, "x || y beside X || Y || ZZ || ZZZ");
    SwCofactorBody<C> cb{dst, ext};
    be.launch(cb, count);
    XyzzBatchAffineBody<C> nb{ext, ext + count * XW, dst, (uint32_t)count, SW_NORM_K};
    be.launch(nb, (count + SW_NORM_K - 1) / SW_NORM_K, 64);
  }
  uint32_t hit_cap = 0;
  be.copy_d2h(&hit_cap, failed, 4);
  if (!hit_cap && digests_host) be.copy_d2h(digests_host, digests, count * 4);
  return hit_cap != 0;
}

}  // namespace
}  // namespace pc

extern "C" {

int pc_hip_sample_generators(pc_ctx* ctx, pc_curve curve, const void* protocol_name, size_t name_len, uint64_t first_index, size_t count,
                             uint32_t* out_digests_host, pc_srs** out) {
  if (!ctx || !out || !count || (!protocol_name && name_len) || !pc_known_curve(curve)) return PC_ERR_INVALID_ARG;
  pc::TeSetupName name;
  if (!name.set(protocol_name, name_len)) return PC_ERR_INVALID_ARG;
  if ((uint64_t)count > ~(uint64_t)0 - first_index) return PC_ERR_INVALID_ARG;      // first_index + count leaves 64 bits
  if (count >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  return key_make(ctx, out, [&]() { return key_create(ctx, curve, count); }, key_free, [&](pc_srs* k) {
    pc::HipBackend& be = ctx->be;
    bool hit_cap = false;
    switch (curve) {
      case PC_CURVE_BLS12_381: hit_cap = pc::sample_run<pc_curve_bls12_381>(be, name, first_index, count, k->bases, out_digests_host); break;
      case PC_CURVE_BN254: hit_cap = pc::sample_run<pc_curve_bn254>(be, name, first_index, count, k->bases, out_digests_host); break;
      case PC_CURVE_PALLAS: hit_cap = pc::sample_run<pc_curve_pallas>(be, name, first_index, count, k->bases, out_digests_host); break;
      case PC_CURVE_BLS12_377: hit_cap = pc::sample_run<pc_curve_bls12_377>(be, name, first_index, count, k->bases, out_digests_host); break;
    }
    if (hit_cap) {
      ctx->last_error = "sample_generators: an index found no point within " + std::to_string(pc::SW_SETUP_MAX_DIGESTS) + " digests";
      return (int)PC_ERR_INTERNAL;
    }
    k->in_subgroup = 1;  // h * P in a group of order h r
    srs_lane(k, 0);      // the first pipeline now, as pc_hip_srs_upload does: no memory for it surfaces here
    return (int)PC_OK;
  });
}

int pc_hip_srs_prefix(pc_ctx* ctx, const pc_srs* src, size_t count, pc_srs** out) {
  if (!ctx || !src || src->ctx != ctx || !out || !count || count > src->n) return PC_ERR_INVALID_ARG;
  return key_make(ctx, out, [&]() { return key_create(ctx, src->curve, count); }, key_free, [&](pc_srs* k) {
    ctx->be.copy_d2d(k->bases, src->bases, count * (size_t)src->aw * 4);
    ctx->be.sync();
    if (src->in_subgroup == 1) k->in_subgroup = 1;
    srs_lane(k, 0);
    return (int)PC_OK;
  });
}

}  // extern "C"
