// The entry points over a scalar field's vector kernels (pc::FrVecOps), written once: the argument checks behind the id check, the
// context's lock, guarded(), the staging.  pc_hip_fr_* / pc_hip_ipa_* (abi_ipa.hip, abi_poly.hip: the field of a pc_curve id) and
// pc_hip_te_fr_* / pc_hip_te_ipa_* (abi_te_ipa.hip: ed_on_bls12_381's) are their id check and one call of these.
#pragma once
#include "abi.hpp"

// the time between the two marks of a call that set exactly two (pc_hip_last_ntt_phases_ms)
inline void one_bracket(pc_ctx* ctx) {
  ctx->ntt_phases[0] = ctx->ntt_phases[1] = 0;
  if (ctx->be.timing && ctx->be.n_ev >= 2) (void)hipEventElapsedTime(&ctx->ntt_phases[0], ctx->be.ev[0], ctx->be.ev[1]);
}

inline int fr_dot_call(pc_ctx* ctx, const pc::FrVecOps& F, const void* a_dev, const void* b_dev, size_t n, void* out_host) {
  if (!ctx || !out_host || (n && (!a_dev || !b_dev))) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    F.fr_dot(ctx->be, (const uint32_t*)a_dev, (const uint32_t*)b_dev, n, (uint32_t*)out_host);
    return (int)PC_OK;
  });
}

inline int ipa_fold_dots_call(pc_ctx* ctx, const pc::FrVecOps& F, void* coeffs_dev, void* z_dev, size_t m, const void* u_host,
                              const void* u_inv_host, void* out_dots_host) {
  if (!ctx || !coeffs_dev || !z_dev || !out_dots_host || !m || (m & (m - 1))) return PC_ERR_INVALID_ARG;
  if ((u_host != nullptr) != (u_inv_host != nullptr)) return PC_ERR_INVALID_ARG;
  if (m >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    F.ipa_fold_dots(ctx->be, (uint32_t*)coeffs_dev, (uint32_t*)z_dev, m, (const uint32_t*)u_host, (const uint32_t*)u_inv_host, (uint32_t*)out_dots_host);
    return (int)PC_OK;
  });
}

inline int fr_powers_call(pc_ctx* ctx, const pc::FrVecOps& F, const void* z_host, size_t n, void* out_dev) {
  if (!ctx || !z_host || (n && !out_dev)) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n) F.fr_powers(ctx->be, (const uint32_t*)z_host, n, (uint32_t*)out_dev);
    return (int)PC_OK;
  });
}

inline int ipa_key_scalars_call(pc_ctx* ctx, const pc::FrVecOps& F, const void* coeffs_dev, size_t m, void* s_dev, size_t n0,
                                const void* fold_u_host, size_t fold_m, void* out_l_dev, void* out_r_dev) {
  if (!ctx || !s_dev || !n0 || (n0 & (n0 - 1))) return PC_ERR_INVALID_ARG;
  if (fold_u_host && (fold_m < 2 || (fold_m & (fold_m - 1)) || fold_m > n0)) return PC_ERR_INVALID_ARG;
  if ((out_l_dev != nullptr) != (out_r_dev != nullptr)) return PC_ERR_INVALID_ARG;
  if (out_l_dev && (!coeffs_dev || m < 2 || (m & (m - 1)) || m > n0)) return PC_ERR_INVALID_ARG;
  if (n0 >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    F.ipa_key_scalars(ctx->be, (const uint32_t*)coeffs_dev, m, (uint32_t*)s_dev, n0, (const uint32_t*)fold_u_host, fold_m, (uint32_t*)out_l_dev,
                      (uint32_t*)out_r_dev);
    return (int)PC_OK;
  });
}

inline int fr_lincomb_call(pc_ctx* ctx, const pc::FrVecOps& F, const void* const* polys, pc_mem where_in, const size_t* lens, size_t k,
                           const void* xi_host, void* out, pc_mem where_out, size_t n_out) {
  constexpr size_t FB = pc::FR_BYTES;
  if (!ctx || (k && (!polys || !lens || !xi_host)) || (n_out && !out)) return PC_ERR_INVALID_ARG;
  if (n_out >= (1ull << 32) || k >= (1ull << 20)) return PC_ERR_TOO_LARGE;
  size_t total = 0;
  for (size_t j = 0; j < k; j++) {
    if (lens[j] >= (1ull << 32)) return PC_ERR_TOO_LARGE;
    if (lens[j] && !polys[j]) return PC_ERR_INVALID_ARG;
    total += lens[j];
  }
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!n_out) return (int)PC_OK;
    // host polynomials are staged back to back in one device buffer
    Staged stage(ctx->be, nullptr, PC_MEM_HOST, where_in == PC_MEM_HOST ? total * FB : 0, false, 0);
    std::vector<uint64_t> addr(k ? k : 1, 0); std::vector<uint32_t> len32(k ? k : 1, 0);
    size_t off = 0;
    for (size_t j = 0; j < k; j++) {
      len32[j] = (uint32_t)lens[j];
      if (where_in == PC_MEM_HOST) {
        if (lens[j]) ctx->be.copy_h2d((char*)stage.dev + off * FB, polys[j], lens[j] * FB);
        addr[j] = (uint64_t)(uintptr_t)((char*)stage.dev + off * FB); off += lens[j];
      } else addr[j] = (uint64_t)(uintptr_t)polys[j];
    }
    // the three small argument arrays side by side in the context's grow-only scratch (three hipMalloc / hipFree pairs per call before)
    const size_t kk = k ? k : 1, o_len = kk * 8, o_xi = (o_len + kk * 4 + 31) & ~(size_t)31;
    char* args = (char*)ctx->be.workspace(o_xi + kk * FB);
    ctx->be.copy_h2d(args, addr.data(), kk * 8);
    ctx->be.copy_h2d(args + o_len, len32.data(), kk * 4);
    if (k) ctx->be.copy_h2d(args + o_xi, xi_host, k * FB);
    Staged sout(ctx->be, out, where_out, n_out * FB, false, 1);
    ctx->be.n_ev = 0; ctx->be.mark();
    F.fr_lincomb(ctx->be, args, args + o_len, args + o_xi, k, sout.dev, n_out);
    ctx->be.mark();
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, n_out * FB); else ctx->be.sync();
    one_bracket(ctx);
    return (int)PC_OK;
  });
}
