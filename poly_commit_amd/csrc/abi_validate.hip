// C ABI of the gfx950 backend (include/pc_hip.h): validation of resident keys, the check() that arkworks runs when it deserializes a key
// with Validate::Yes (poly-commit/src/kzg10/data_structures.rs:41-49, :106-108) -- per point is_on_curve() and
// is_in_correct_subgroup_assuming_on_curve().  The kernels are validate.hpp's, one lane per point; this unit instantiates them for the
// four curves of pc_curve and for G2 of BLS12-381 itself: nothing else in the library needs them.
#include "abi.hpp"
#include "setup_constants.h"
#include "validate.hpp"

namespace pc {
namespace {

constexpr unsigned CHECK_ALL = PC_HIP_CHECK_ON_CURVE | PC_HIP_CHECK_SUBGROUP;

// PC_HIP_SUBGROUP_LADDER=1: the plain ladder by r on the BLS12 curves too (read at every call: one process can time both)
bool force_ladder() { const char* e = getenv("PC_HIP_SUBGROUP_LADDER"); return e && atoi(e) != 0; }

// The measured decision, per curve: true where tools/validate_timing.py found the fast test faster than the plain ladder in the same
// run (profiles/validate_timing.jsonl: plain ladder / fast test = 2.2 at 2^16 points and 3.0 at 2^20 on both curves).
// A curve without an entry, or with false, takes the plain ladder.
template <class C> struct SubgroupFastDefault { static constexpr bool value = false; };
template <> struct SubgroupFastDefault<pc_curve_bls12_381> { static constexpr bool value = true; };
template <> struct SubgroupFastDefault<pc_curve_bls12_377> { static constexpr bool value = true; };

// flags[i] of `what` for the G1 points at pts.  false: nothing was launched and every point passes (the subgroup test alone on a curve
// of cofactor 1)
template <class C>
bool g1_flags(HipBackend& be, const uint32_t* pts, size_t count, unsigned what, uint32_t* flags) {
  constexpr bool COFACTOR_ONE = pc_cofactor_constants<C>::COFACTOR_BITS == 1;
  const uint32_t* gate = nullptr;
  if (what & PC_HIP_CHECK_ON_CURVE) {
    SwOnCurveBody<C> b{pts, flags};
    be.launch(b, count);
    gate = flags;
  }
  if (what & PC_HIP_CHECK_SUBGROUP) {
    if constexpr (COFACTOR_ONE) return gate != nullptr;
    if constexpr (SubgroupFastDefault<C>::value) {
      if (!force_ladder()) {
        Bls12SubgroupBody<C> b{pts, flags, gate};
        be.launch(b, count);
        return true;
      }
    }
    SwSubgroupLadderBody<C> b;
    b.key = pts; b.flags = flags; b.gate = gate; b.set_order();
    be.launch(b, count);
  }
  return true;
}

void g2_flags(HipBackend& be, const uint32_t* pts, size_t count, unsigned what, uint32_t* flags) {
  typedef pc_curve_bls12_381 C;
  const uint32_t* gate = nullptr;
  if (what & PC_HIP_CHECK_ON_CURVE) {
    G2OnCurveBody<C> b{pts, flags};
    be.launch(b, count);
    gate = flags;
  }
  if (what & PC_HIP_CHECK_SUBGROUP) {
    G2SubgroupBody<C> b;
    b.key = pts; b.flags = flags; b.gate = gate; b.set_order();
    be.launch(b, count);
  }
}

// The query over `count` points of a key (inside guarded()): make(flags) launches the passes (false: every point passes), the tally
// counts on the device
template <class Make>
int check_points(pc_ctx* ctx, size_t count, size_t* out_bad, size_t* out_first_bad, uint8_t* out_ok_host, Make make) {
  HipBackend& be = ctx->be;
  // flags | the counter and the minimum | one byte per point
  CallBuf ws(be, 1, count * 4 + 8 + count);
  uint32_t* flags = (uint32_t*)ws.dev;
  uint32_t* tally = flags + count;
  uint8_t* ok = (uint8_t*)(tally + 2);
  if (!make(flags)) {
    *out_bad = 0;
    if (out_ok_host) memset(out_ok_host, 1, count);
    return PC_OK;
  }
  be.memset(tally, 0, 4);
  be.memset(tally + 1, 0xff, 4);
  ValidateTallyBody t{flags, out_ok_host ? ok : nullptr, tally, tally + 1};
  be.launch(t, count);
  uint32_t got[2];
  be.copy_d2h(got, tally, sizeof got);
  if (out_ok_host) be.copy_d2h(out_ok_host, ok, count);
  *out_bad = got[0];
  if (out_first_bad) *out_first_bad = got[0] ? got[1] : 0;
  return PC_OK;
}

bool check_args(const pc_ctx* ctx, const pc_key_base* k, size_t offset, size_t count, unsigned what, const size_t* out_bad) {
  return ctx && k && k->ctx == ctx && out_bad && offset <= k->n && count <= k->n - offset && what && !(what & ~CHECK_ALL);
}

}  // namespace
}  // namespace pc

extern "C" {

int pc_hip_srs_check(pc_ctx* ctx, const pc_srs* srs, size_t offset, size_t count, unsigned what, size_t* out_bad, size_t* out_first_bad,
                     uint8_t* out_ok_host) {
  if (!pc::check_args(ctx, srs, offset, count, what, out_bad)) return PC_ERR_INVALID_ARG;
  *out_bad = 0;
  if (out_first_bad) *out_first_bad = 0;
  if (!count) return PC_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const uint32_t* pts = srs->bases + offset * (size_t)srs->aw;
    return pc::check_points(ctx, count, out_bad, out_first_bad, out_ok_host, [&](uint32_t* flags) {
      switch (srs->curve) {
        case PC_CURVE_BLS12_381: return pc::g1_flags<pc_curve_bls12_381>(ctx->be, pts, count, what, flags);
        case PC_CURVE_BN254: return pc::g1_flags<pc_curve_bn254>(ctx->be, pts, count, what, flags);
        case PC_CURVE_PALLAS: return pc::g1_flags<pc_curve_pallas>(ctx->be, pts, count, what, flags);
        case PC_CURVE_BLS12_377: return pc::g1_flags<pc_curve_bls12_377>(ctx->be, pts, count, what, flags);
      }
      throw std::invalid_argument("unknown curve id");
    });
  });
}

int pc_hip_srs_in_subgroup(pc_ctx* ctx, pc_srs* srs, int* out) {
  if (!ctx || !srs || srs->ctx != ctx || !out) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (srs->in_subgroup < 0) {
    size_t bad = 0;
    if (int rc = pc_hip_srs_check(ctx, srs, 0, srs->n, PC_HIP_CHECK_SUBGROUP, &bad, nullptr, nullptr)) return rc;
    srs->in_subgroup = bad ? 0 : 1;
  }
  *out = srs->in_subgroup;
  return PC_OK;
}

int pc_hip_srs_load_serialized_ex(pc_ctx* ctx, pc_curve curve, const void* bytes, size_t n_bytes, int compressed, size_t max_points,
                                  unsigned validate, pc_srs** out, size_t* out_points, size_t* out_bytes_consumed) {
  if (!ctx || !out || (validate & ~pc::CHECK_ALL)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  // the decoder tests the curve equation whatever the caller asks for: PC_HIP_CHECK_ON_CURVE adds nothing to it
  size_t points = 0, consumed = 0;
  if (int rc = pc_hip_srs_load_serialized(ctx, curve, bytes, n_bytes, compressed, max_points, out, &points, &consumed)) return rc;
  if (validate & PC_HIP_CHECK_SUBGROUP) {
    size_t bad = 0, first = 0;
    int rc = pc_hip_srs_check(ctx, *out, 0, (*out)->n, PC_HIP_CHECK_SUBGROUP, &bad, &first, nullptr);
    if (rc == PC_OK && bad) {
      ctx->last_error = std::to_string(bad) + " serialized point(s) are not in the prime-order subgroup, the first at index " + std::to_string(first);
      rc = PC_ERR_INVALID_ARG;
    }
    if (rc != PC_OK) { pc_hip_srs_free(*out); *out = nullptr; return rc; }
    (*out)->in_subgroup = 1;
  }
  if (out_points) *out_points = points;
  if (out_bytes_consumed) *out_bytes_consumed = consumed;
  return PC_OK;
}

int pc_hip_g2_srs_check(pc_ctx* ctx, const pc_g2_srs* srs, size_t offset, size_t count, unsigned what, size_t* out_bad,
                        size_t* out_first_bad, uint8_t* out_ok_host) {
  if (!pc::check_args(ctx, srs, offset, count, what, out_bad) || srs->curve != PC_CURVE_BLS12_381) return PC_ERR_INVALID_ARG;
  *out_bad = 0;
  if (out_first_bad) *out_first_bad = 0;
  if (!count) return PC_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const uint32_t* pts = srs->bases + offset * (size_t)srs->aw;
    return pc::check_points(ctx, count, out_bad, out_first_bad, out_ok_host, [&](uint32_t* flags) {
      pc::g2_flags(ctx->be, pts, count, what, flags);
      return true;
    });
  });
}

}  // extern "C"
