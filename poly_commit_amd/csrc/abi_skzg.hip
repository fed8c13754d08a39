// C ABI of the gfx950 backend (include/pc_hip.h): streaming_kzg -- the folding tree, the division by a vanishing polynomial, the
// multi-point openings of time.rs and the commit_folding / open_folding of space.rs against one resident key.
// The kernels are csrc/skzg.hpp (through FieldOps); the MSMs, the combination of polynomials and the key are the existing entry
// points' (pc_hip_msm, pc_hip_msm_batch, pc_hip_fr_lincomb), called under the context's recursive lock.
#include <string.h>
#include "abi.hpp"

namespace {

constexpr size_t EB = 32;                      // bytes of one Fr
constexpr size_t MAX_DEPTH = PC_HIP_MAX_FOLD_DEPTH;

// L_i = ceil(n / 2^i) and the element offset of level i in a buffer that holds the levels 1 .. depth back to back
struct Levels {
  std::vector<uint32_t> len; std::vector<uint64_t> off; size_t total = 0;
  Levels(size_t n, size_t depth) : len(depth), off(depth) {
    size_t l = n;
    for (size_t i = 0; i < depth; i++) { l = (l + 1) / 2; len[i] = (uint32_t)l; off[i] = total; total += l; }
  }
};

void identity(const pc_srs* srs, void* out_xy, int* out_is_infinity) {
  memset(out_xy, 0, (size_t)srs->aw * 4);
  if (out_is_infinity) *out_is_infinity = 1;
}

// a key of another context, or fewer than `need` points from base_offset on (looked at after the checks on the arguments alone)
bool key_too_short(const pc_ctx* ctx, const pc_srs* srs, size_t base_offset, size_t need) {
  return srs->ctx != ctx || base_offset > srs->n || need > srs->n - base_offset;
}

// proof = sum_d q[d] * bases[base_offset + d], q = p div Z, and r = p mod Z for a polynomial on the device (n >= k, checked).
// arena: 1 + (n - k) coefficients followed by the division's scratch
int open_multi_dev(pc_ctx* ctx, pc_srs* srs, size_t base_offset, const uint32_t* p, size_t n, const uint32_t* z, uint32_t k, void* rem_host,
                   char* arena, void* out_xy, int* out_is_infinity) {
  uint32_t* q = (uint32_t*)arena + 8;
  std::vector<uint32_t> rem((size_t)k * 8);
  const pc::SkzgDivLevel lv{p, (uint32_t)n, q};
  ctx->skzg_launches[1] += pc::field_ops(srs->curve).div_multi(ctx->be, &lv, 1, z, k, rem.data(), arena + (1 + (n - k)) * EB, scan_fan());
  if (rem_host) memcpy(rem_host, rem.data(), (size_t)k * EB);
  if (n == k) { identity(srs, out_xy, out_is_infinity); return PC_OK; }
  return pc_hip_msm(ctx, srs, base_offset, q, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n - k, out_xy, out_is_infinity);
}
size_t open_multi_arena(size_t n, uint32_t k) { return (1 + (n - k)) * EB + pc::skzg_div_scratch_bytes(n, 1, k); }

}  // namespace

extern "C" {

int pc_hip_fold_tree(pc_ctx* ctx, pc_curve field_of, const void* coeffs, pc_mem where_in, size_t n, const void* challenges_host, size_t depth,
                     void* out_dev, size_t out_capacity_elems, size_t* level_offsets_host) {
  if (!ctx || !pc_known_curve(field_of) || !coeffs || !challenges_host || !out_dev || !level_offsets_host || !n || !depth) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32) || depth > MAX_DEPTH) return PC_ERR_TOO_LARGE;
  const Levels L(n, depth);
  if (out_capacity_elems < L.total) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sin(ctx->be, coeffs, where_in, n * EB, true, 0);
    ctx->skzg_launches[0] = pc::field_ops(field_of).fold_tree(ctx->be, (const uint32_t*)sin.dev, n, (const uint32_t*)challenges_host, (uint32_t)depth,
                                                              (uint32_t*)out_dev, L.off.data());
    ctx->skzg_launches[1] = 0;
    ctx->be.sync();
    for (size_t i = 0; i < depth; i++) level_offsets_host[i] = (size_t)L.off[i];
    return (int)PC_OK;
  });
}

int pc_hip_poly_div_multi(pc_ctx* ctx, pc_curve field_of, const void* coeffs, pc_mem where_in, size_t n, const void* points_host, size_t k,
                          void* quotient_out, pc_mem where_out, void* remainder_host) {
  if (!ctx || !pc_known_curve(field_of) || !coeffs || !points_host || !remainder_host || !n || !k) return PC_ERR_INVALID_ARG;
  if (k > PC_HIP_MAX_EVAL_POINTS || n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const size_t m = n > k ? n - k : 0;
    Staged sin(ctx->be, coeffs, where_in, n * EB, true, 0);
    CallBuf buf(ctx->be, 1, (1 + m) * EB + pc::skzg_div_scratch_bytes(n, 1, (uint32_t)k));
    uint32_t* q = (uint32_t*)buf.dev + 8;
    const pc::SkzgDivLevel lv{(const uint32_t*)sin.dev, (uint32_t)n, q};
    ctx->skzg_launches[0] = 0;
    ctx->skzg_launches[1] = pc::field_ops(field_of).div_multi(ctx->be, &lv, 1, (const uint32_t*)points_host, (uint32_t)k, (uint32_t*)remainder_host,
                                                              (char*)buf.dev + (1 + m) * EB, scan_fan());
    if (quotient_out && m) {
      if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(quotient_out, q, m * EB);
      else { ctx->be.copy_d2d(quotient_out, q, m * EB); ctx->be.sync(); }
    }
    return (int)PC_OK;
  });
}

int pc_hip_kzg_open_multi(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* coeffs, pc_mem where, size_t n, const void* points_host,
                          size_t k, void* remainder_host, void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !coeffs || !points_host || !out_xy || !n || !k) return PC_ERR_INVALID_ARG;
  if (k > PC_HIP_MAX_EVAL_POINTS || n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  if (n < k || key_too_short(ctx, srs, base_offset, n - k)) return PC_ERR_INVALID_ARG;      // space.rs:104-106 asserts the first; the time form's n <= k is the mirror's
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sin(ctx->be, coeffs, where, n * EB, true, 0);
    CallBuf buf(ctx->be, 1, open_multi_arena(n, (uint32_t)k));
    ctx->skzg_launches[0] = ctx->skzg_launches[1] = 0;
    return open_multi_dev(ctx, srs, base_offset, (const uint32_t*)sin.dev, n, (const uint32_t*)points_host, (uint32_t)k, remainder_host, (char*)buf.dev,
                          out_xy, out_is_infinity);
  });
}

int pc_hip_kzg_batch_open_multi(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* const* polys, pc_mem where, const size_t* lens,
                                size_t count, const void* points_host, size_t k, const void* eta_host, void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !polys || !lens || !points_host || !eta_host || !out_xy || !count || !k) return PC_ERR_INVALID_ARG;
  if (k > PC_HIP_MAX_EVAL_POINTS || count >= (1ull << 20)) return PC_ERR_TOO_LARGE;
  size_t n = 0;
  for (size_t j = 0; j < count; j++) {
    if (lens[j] >= (1ull << 32)) return PC_ERR_TOO_LARGE;
    if (lens[j] && !polys[j]) return PC_ERR_INVALID_ARG;
    n = std::max(n, lens[j]);
  }
  if (key_too_short(ctx, srs, base_offset, n > k ? n - k : 0)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n <= k) { identity(srs, out_xy, out_is_infinity); return (int)PC_OK; }                  // time.rs:134-136: a quotient of no coefficients
    const pc::CurveOps& C = pc::curve_ops(srs->curve);
    std::vector<uint32_t> xi(count * 8);                                                         // 1, eta, eta^2, ... (mod.rs:302-310)
    C.fr_one(xi.data());
    for (size_t j = 1; j < count; j++) C.fr_mul(&xi[(j - 1) * 8], (const uint32_t*)eta_host, &xi[j * 8]);
    CallBuf buf(ctx->be, 1, n * EB + open_multi_arena(n, (uint32_t)k));
    int rc = pc_hip_fr_lincomb(ctx, srs->curve, polys, where, lens, count, xi.data(), buf.dev, PC_MEM_DEVICE, n);
    if (rc != PC_OK) return rc;
    ctx->skzg_launches[0] = 0; ctx->skzg_launches[1] = 1;
    return open_multi_dev(ctx, srs, base_offset, (const uint32_t*)buf.dev, n, (const uint32_t*)points_host, (uint32_t)k, nullptr, (char*)buf.dev + n * EB,
                          out_xy, out_is_infinity);
  });
}

int pc_hip_kzg_commit_folding(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* coeffs, pc_mem where, size_t n,
                              const void* challenges_host, size_t depth, void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !coeffs || !challenges_host || !out_xy || !n || !depth) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32) || depth > MAX_DEPTH) return PC_ERR_TOO_LARGE;
  const Levels L(n, depth);
  if (key_too_short(ctx, srs, base_offset, L.len[0])) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sin(ctx->be, coeffs, where, n * EB, true, 0);
    CallBuf buf(ctx->be, 1, L.total * EB);
    ctx->skzg_launches[0] = pc::field_ops(srs->curve).fold_tree(ctx->be, (const uint32_t*)sin.dev, n, (const uint32_t*)challenges_host, (uint32_t)depth,
                                                                (uint32_t*)buf.dev, L.off.data());
    ctx->skzg_launches[1] = 0;
    ctx->be.sync();
    // one MSM per level over the key's pipelines, each level's accumulation beside the tail of the one before (pc_hip_msm_batch)
    std::vector<const void*> ptrs(depth); std::vector<size_t> lens(depth), offs(depth, base_offset);
    for (size_t i = 0; i < depth; i++) { ptrs[i] = (const char*)buf.dev + L.off[i] * EB; lens[i] = L.len[i]; }
    return pc_hip_msm_batch(ctx, srs, offs.data(), ptrs.data(), lens.data(), depth, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, out_xy, out_is_infinity);
  });
}

int pc_hip_kzg_open_folding(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* coeffs, pc_mem where, size_t n,
                            const void* challenges_host, size_t depth, const void* points_host, size_t k, const void* etas_host,
                            void* remainders_host, void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !coeffs || !challenges_host || !points_host || !etas_host || !remainders_host || !out_xy || !n || !depth || !k)
    return PC_ERR_INVALID_ARG;
  if (k > PC_HIP_MAX_EVAL_POINTS || n >= (1ull << 32) || depth > MAX_DEPTH) return PC_ERR_TOO_LARGE;
  const Levels L(n, depth);
  const size_t m = L.len[0] > k ? L.len[0] - k : 0;                                               // pairs of the one MSM
  if (key_too_short(ctx, srs, base_offset, m)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const pc::FieldOps& F = pc::field_ops(srs->curve);
    // arena: the tree | per level one slot and its quotient | the combined quotient | the division's scratch
    std::vector<size_t> qoff(depth); size_t qtotal = 0;
    for (size_t i = 0; i < depth; i++) { qoff[i] = qtotal + 1; qtotal += 1 + (L.len[i] > k ? L.len[i] - k : 0); }
    Staged sin(ctx->be, coeffs, where, n * EB, true, 0);
    CallBuf buf(ctx->be, 1, (L.total + qtotal + m) * EB + pc::skzg_div_scratch_bytes(L.len[0], depth, (uint32_t)k));
    char* tree = (char*)buf.dev; char* quot = tree + L.total * EB; char* comb = quot + qtotal * EB; char* scratch = comb + m * EB;
    ctx->skzg_launches[0] = F.fold_tree(ctx->be, (const uint32_t*)sin.dev, n, (const uint32_t*)challenges_host, (uint32_t)depth, (uint32_t*)tree, L.off.data());
    std::vector<pc::SkzgDivLevel> lv(depth);
    for (size_t i = 0; i < depth; i++) lv[i] = pc::SkzgDivLevel{(const uint32_t*)(tree + L.off[i] * EB), L.len[i], (uint32_t*)(quot + qoff[i] * EB)};
    ctx->skzg_launches[1] = F.div_multi(ctx->be, lv.data(), depth, (const uint32_t*)points_host, (uint32_t)k, (uint32_t*)remainders_host, scratch, scan_fan());
    if (!m) { identity(srs, out_xy, out_is_infinity); return (int)PC_OK; }                       // every quotient is empty
    // s[d] = sum_i eta_{i-1} * (f_i div Z)[d] (space.rs:244-252): the level quotients have different lengths
    std::vector<const void*> ptrs(depth); std::vector<size_t> lens(depth);
    for (size_t i = 0; i < depth; i++) { ptrs[i] = lv[i].q; lens[i] = L.len[i] > k ? L.len[i] - k : 0; }
    int rc = pc_hip_fr_lincomb(ctx, srs->curve, ptrs.data(), PC_MEM_DEVICE, lens.data(), depth, etas_host, comb, PC_MEM_DEVICE, m);
    if (rc != PC_OK) return rc;
    ctx->skzg_launches[1] += 1;
    return pc_hip_msm(ctx, srs, base_offset, comb, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, m, out_xy, out_is_infinity);
  });
}

int pc_hip_last_skzg_launches(const pc_ctx* ctx, unsigned out[2]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  out[0] = ctx->skzg_launches[0]; out[1] = ctx->skzg_launches[1];
  return PC_OK;
}

}  // extern "C"
