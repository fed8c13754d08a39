// C ABI of the gfx950 backend (include/pc_hip.h): InnerProductArgPC::setup and trim over ed_on_bls12_381 (JubJub) on the device --
// sample_generators (ipa_pc/mod.rs:302-325) as a new resident key, and trim's prefix of a key (:384).  The kernels are te_setup.hpp's
// (digest, from_random_bytes, cofactor: one lane per index) and te.hpp's batch normalisation; the key object is key.hpp's.
#include <vector>
#include "abi_te.hpp"
#include "te_setup.hpp"

using pc::TeC;
using pc::TE_AW;

extern "C" {

int pc_hip_te_sample_generators(pc_ctx* ctx, pc_te_curve curve, const void* protocol_name, size_t name_len, uint64_t first_index, size_t count,
                                uint32_t* out_digests_host, pc_te_srs** out) {
  if (!ctx || !out || !count || (!protocol_name && name_len)) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  pc::TeSampleBody<TeC> body;
  if (!body.name.set(protocol_name, name_len)) return PC_ERR_INVALID_ARG;
  if ((uint64_t)count > ~(uint64_t)0 - first_index) return PC_ERR_INVALID_ARG;      // first_index + count leaves 64 bits
  if (count >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  return key_make(ctx, out, [&]() { return te_key_create(ctx, curve, count, (size_t)TE_AW * 4); }, te_key_free, [&](pc_te_srs* k) {
    pc::HipBackend& be = ctx->be;
    // the points in extended coordinates | the prefix products of the normalisation | the digest counts | the flag of the cap
    const pc::TeNormBuf ws = pc::te_norm_buf(be, count, count + 1);
    uint32_t* digests = ws.extra;
    uint32_t* failed = digests + count;
    be.memset(failed, 0, 4);
    body.first = first_index; body.ext = ws.ext; body.digests = digests; body.failed = failed;
    be.launch(body, count);
    pc::te_normalise(be, ws.ext, ws.scratch, k->bases, count);
    uint32_t hit_cap = 0;
    be.copy_d2h(&hit_cap, failed, 4);
    if (hit_cap) {
      ctx->last_error = "sample_generators: an index found no point within " + std::to_string(pc::TE_SETUP_MAX_DIGESTS) + " digests";
      return (int)PC_ERR_INTERNAL;
    }
    if (out_digests_host) be.copy_d2h(out_digests_host, digests, count * 4);
    k->in_subgroup = 1;      // 8 * P in a group of order 8 r
    return (int)PC_OK;
  });
}

int pc_hip_te_srs_prefix(pc_ctx* ctx, const pc_te_srs* src, size_t count, pc_te_srs** out) {
  if (!ctx || !src || src->ctx != ctx || !out || !count || count > src->n) return PC_ERR_INVALID_ARG;
  return key_make(ctx, out, [&]() { return te_key_create(ctx, src->te_curve, count, (size_t)TE_AW * 4); }, te_key_free, [&](pc_te_srs* k) {
    ctx->be.copy_d2d(k->bases, src->bases, count * (size_t)TE_AW * 4);
    ctx->be.sync();
    if (src->in_subgroup == 1) k->in_subgroup = 1;
    return (int)PC_OK;
  });
}

}  // extern "C"
