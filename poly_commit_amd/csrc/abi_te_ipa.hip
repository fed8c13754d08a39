// C ABI of the gfx950 backend (include/pc_hip.h): InnerProductArgPC::open over ed_on_bls12_381 (JubJub) on the device -- the vector
// kernels of the halving rounds over the curve's 252-bit scalar field, and the rounds as one call (ipa_pc/mod.rs:664-711).
// With them the two vector kernels of HyraxPC::open over that field, fr_lincomb and fr_dot (hyrax/mod.rs:347,356,391).
// This unit instantiates the members of FieldOpsImpl that the rounds and Hyrax need for that field and no other: its 2-adicity is 1, there is
// no NTT over it (and nothing of a FieldOps table: pc_curve keeps its four ids).  The group side is abi_te.hip's, through the C ABI.
#include <chrono>
#include <string.h>
#include "abi.hpp"
#include "field_ops_impl.hpp"
#include "host_tail.hpp"
#include "te_constants.h"

namespace {
typedef pc_ed_on_bls12_381_fr TeFrP;
typedef pc::FieldOpsImpl<TeFrP> TeFr;
typedef pc::host64::F64<TeFrP> TeFr64;
constexpr size_t TE_POINT_BYTES = 2 * (size_t)pc_te_ed_on_bls12_381::FqP::N * 4, TE_FR_BYTES = (size_t)TeFrP::N * 4;
int te_curve_check(pc_te_curve curve) { return curve == PC_TE_ED_ON_BLS12_381 ? PC_OK : PC_ERR_INVALID_ARG; }
}  // namespace

extern "C" {

int pc_hip_te_fr_powers(pc_ctx* ctx, pc_te_curve curve, const void* z_host, size_t n, void* out_dev) {
  if (!ctx || !z_host || (n && !out_dev)) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n) TeFr::fr_powers(ctx->be, (const uint32_t*)z_host, n, (uint32_t*)out_dev);
    return (int)PC_OK;
  });
}

// <a, b> and sum_j xi[j] * polys[j] over the curve's scalar field: HyraxPC::open's <lt, r> and t.row_mul(l) (hyrax/mod.rs:347,356,391)
int pc_hip_te_fr_dot(pc_ctx* ctx, pc_te_curve curve, const void* a_dev, const void* b_dev, size_t n, void* out_host) {
  if (!ctx || !out_host || (n && (!a_dev || !b_dev))) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    TeFr::fr_dot(ctx->be, (const uint32_t*)a_dev, (const uint32_t*)b_dev, n, (uint32_t*)out_host);
    return (int)PC_OK;
  });
}

int pc_hip_te_fr_lincomb(pc_ctx* ctx, pc_te_curve curve, const void* const* polys, pc_mem where_in, const size_t* lens,
                         size_t k, const void* xi_host, void* out, pc_mem where_out, size_t n_out) {
  if (!ctx || (k && (!polys || !lens || !xi_host)) || (n_out && !out)) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
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
    // host vectors are staged back to back in one device buffer; the three small argument arrays side by side in the context's scratch
    Staged stage(ctx->be, nullptr, PC_MEM_HOST, where_in == PC_MEM_HOST ? total * TE_FR_BYTES : 0, false, 0);
    std::vector<uint64_t> addr(k ? k : 1, 0); std::vector<uint32_t> len32(k ? k : 1, 0);
    size_t off = 0;
    for (size_t j = 0; j < k; j++) {
      len32[j] = (uint32_t)lens[j];
      if (where_in == PC_MEM_HOST) {
        if (lens[j]) ctx->be.copy_h2d((char*)stage.dev + off * TE_FR_BYTES, polys[j], lens[j] * TE_FR_BYTES);
        addr[j] = (uint64_t)(uintptr_t)((char*)stage.dev + off * TE_FR_BYTES); off += lens[j];
      } else addr[j] = (uint64_t)(uintptr_t)polys[j];
    }
    const size_t kk = k ? k : 1, o_len = kk * 8, o_xi = (o_len + kk * 4 + 31) & ~(size_t)31;
    char* args = (char*)ctx->be.workspace(o_xi + kk * TE_FR_BYTES);
    ctx->be.copy_h2d(args, addr.data(), kk * 8);
    ctx->be.copy_h2d(args + o_len, len32.data(), kk * 4);
    if (k) ctx->be.copy_h2d(args + o_xi, xi_host, k * TE_FR_BYTES);
    Staged sout(ctx->be, out, where_out, n_out * TE_FR_BYTES, false, 1);
    TeFr::fr_lincomb(ctx->be, args, args + o_len, args + o_xi, k, sout.dev, n_out);
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, n_out * TE_FR_BYTES); else ctx->be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_te_ipa_fold_dots(pc_ctx* ctx, pc_te_curve curve, void* coeffs_dev, void* z_dev, size_t m, const void* u_host, const void* u_inv_host,
                            void* out_dots_host) {
  if (!ctx || !coeffs_dev || !z_dev || !out_dots_host || !m || (m & (m - 1))) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  if ((u_host != nullptr) != (u_inv_host != nullptr)) return PC_ERR_INVALID_ARG;
  if (m >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    TeFr::ipa_fold_dots(ctx->be, (uint32_t*)coeffs_dev, (uint32_t*)z_dev, m, (const uint32_t*)u_host, (const uint32_t*)u_inv_host, (uint32_t*)out_dots_host);
    return (int)PC_OK;
  });
}

int pc_hip_te_ipa_key_scalars(pc_ctx* ctx, pc_te_curve curve, const void* coeffs_dev, size_t m, void* s_dev, size_t n0,
                              const void* fold_u_host, size_t fold_m, void* out_l_dev, void* out_r_dev) {
  if (!ctx || !s_dev || !n0 || (n0 & (n0 - 1))) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  if (fold_u_host && (fold_m < 2 || (fold_m & (fold_m - 1)) || fold_m > n0)) return PC_ERR_INVALID_ARG;
  if ((out_l_dev != nullptr) != (out_r_dev != nullptr)) return PC_ERR_INVALID_ARG;
  if (out_l_dev && (!coeffs_dev || m < 2 || (m & (m - 1)) || m > n0)) return PC_ERR_INVALID_ARG;
  if (n0 >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    TeFr::ipa_key_scalars(ctx->be, (const uint32_t*)coeffs_dev, m, (uint32_t*)s_dev, n0, (const uint32_t*)fold_u_host, fold_m, (uint32_t*)out_l_dev,
                          (uint32_t*)out_r_dev);
    return (int)PC_OK;
  });
}

// The halving loop of InnerProductArgPC::open as ONE call, in the order pc_hip_ipa_open_rounds runs it for the pc_curve curves: plain
// launches, blocking MSMs on the key's one pipeline.  The first fold is out of place (the committer key stays; from its fold table when
// it has one and n is its length), later folds are in place on the working key.  From `fixed_key_below` points on the key stays fixed
// and the per-base factors carry the folds -- only on a committer key whose points all lie in the prime-order subgroup
// (pc_hip_te_srs_in_subgroup, asked here once per key): the factors are products modulo r.  On any other key every round folds.
int pc_hip_te_ipa_open_rounds(pc_ctx* ctx, const pc_te_srs* comm_key, void* coeffs_dev, size_t n, const void* point_host, const void* h_prime_xy_host,
                              pc_ipa_challenge_fn next_challenge, void* user, size_t fixed_key_below,
                              void* out_l_vec_xy, void* out_r_vec_xy, void* out_final_key_xy, void* out_c_host, float* out_round_ms, float* out_fold_ms) {
  pc_te_srs* root = const_cast<pc_te_srs*>(comm_key);
  if (!ctx || !root || root->ctx != ctx || !coeffs_dev || !n || (n & (n - 1)) || n > root->n || !point_host || !h_prime_xy_host || !next_challenge ||
      !out_final_key_xy || !out_c_host || (n > 1 && (!out_l_vec_xy || !out_r_vec_xy))) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  const pc_te_curve curve = root->te_curve;
  if (!fixed_key_below) fixed_key_below = (size_t)1 << 16;      // the default; any value below 2: the key is folded in every round
  pc_te_srs* srs = root; bool owned = false;
  struct KeyGuard { pc_te_srs*& k; bool& owned; ~KeyGuard() { if (owned && k) pc_hip_te_srs_free(k); } } key_guard{srs, owned};
  void* z = nullptr; void* s_dev = nullptr; char* alr = nullptr;
  int rc = guarded(ctx, [&]() { z = ipa_buffer(ctx, 0, n * TE_FR_BYTES); return (int)PC_OK; });
  if (rc != PC_OK) return rc;
  char* c = (char*)coeffs_dev;
  rc = pc_hip_te_fr_powers(ctx, curve, point_host, n, z);                                          // z = (1, point, point^2, ..)   :641-649
  uint32_t dots[2][8];
  if (rc == PC_OK) rc = pc_hip_te_ipa_fold_dots(ctx, curve, c, z, n, nullptr, nullptr, dots);      // the inner products of the first round
  size_t n0 = 0;
  bool folds_only = false;                                                                         // the key failed the subgroup check
  uint32_t u_prev[8], u[8], ui[8], one[8];
  bool have_u_prev = false;
  TeFr64::one().store(one);
  uint32_t pts[4 * 16];                                                                            // ml | hl | mr | hr
  uint32_t* ml = pts; uint32_t* hl = ml + 16; uint32_t* mr = hl + 16; uint32_t* hr = mr + 16;
  size_t round = 0;
  using clk = std::chrono::steady_clock;
  for (size_t m = n; rc == PC_OK && m > 1; m /= 2, round++) {
    const auto t_round = clk::now();
    const size_t h = m / 2;
    if (!n0 && !folds_only && m <= fixed_key_below) {                                              // from here on key[0 .. n0) stays fixed
      int inside = 0;
      rc = pc_hip_te_srs_in_subgroup(ctx, root, &inside);
      if (rc != PC_OK) break;
      if (!inside) folds_only = true;
      else {
        n0 = m;
        rc = guarded(ctx, [&]() { s_dev = ipa_buffer(ctx, 1, n0 * TE_FR_BYTES); alr = (char*)ipa_buffer(ctx, 2, 2 * n0 * TE_FR_BYTES); return (int)PC_OK; });
        if (rc == PC_OK) rc = pc_hip_te_fr_powers(ctx, curve, one, n0, s_dev);                     // s = (1, 1, ..)
        if (rc != PC_OK) break;
      }
    }
    // l = cm_commit(key_l, coeffs_r) + h' <coeffs_r, z_l>;  r = cm_commit(key_r, coeffs_l) + h' <coeffs_l, z_r>          :666-675
    if (n0) {
      rc = pc_hip_te_ipa_key_scalars(ctx, curve, c, m, s_dev, n0, have_u_prev ? u_prev : nullptr, have_u_prev ? 2 * m : 0, alr, alr + TE_FR_BYTES * n0);
      if (rc == PC_OK) rc = pc_hip_te_msm(ctx, srs, 0, alr, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n0, ml, nullptr);
      if (rc == PC_OK) rc = pc_hip_te_msm(ctx, srs, 0, alr + TE_FR_BYTES * n0, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n0, mr, nullptr);
    } else {
      rc = pc_hip_te_msm(ctx, srs, 0, c + TE_FR_BYTES * h, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, h, ml, nullptr);
      if (rc == PC_OK) rc = pc_hip_te_msm(ctx, srs, h, c, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, h, mr, nullptr);
    }
    if (rc == PC_OK) rc = pc_hip_te_point_mul(curve, h_prime_xy_host, dots[0], hl);                // h' * <.., ..>, one point each
    if (rc == PC_OK) rc = pc_hip_te_point_mul(curve, h_prime_xy_host, dots[1], hr);
    if (rc != PC_OK) break;
    uint32_t* l = (uint32_t*)((char*)out_l_vec_xy + round * TE_POINT_BYTES); uint32_t* r = (uint32_t*)((char*)out_r_vec_xy + round * TE_POINT_BYTES);
    pc_hip_te_points_sum(curve, ml, 2, l);
    pc_hip_te_points_sum(curve, mr, 2, r);
    next_challenge(user, l, r, u);                                                                 // :681-689, the caller's transcript
    TeFr64::load(u).inv().store(ui);                                                               // (0 -> 0, as pc_hip_ipa_open_rounds has it)
    rc = pc_hip_te_ipa_fold_dots(ctx, curve, c, z, h, u, ui, dots);                                // :691-697 + the next round's inner products
    if (rc != PC_OK) break;
    const auto t_fold = clk::now();
    bool folded = false;
    if (n0) { memcpy(u_prev, u, TE_FR_BYTES); have_u_prev = true; }                                // applied to the factors at the top of the next round
    else if (owned) { rc = pc_hip_te_ec_fold(ctx, srs, h, u); folded = true; }                     // key_l += u key_r, normalised          :699-707
    else {
      pc_te_srs* work = nullptr;
      rc = pc_hip_te_ec_fold_from(ctx, srs, h, u, &work);                                          // the same fold, out of place: the committer key stays
      if (rc == PC_OK) { srs = work; owned = true; }
      folded = true;
    }
    const auto t_end = clk::now();
    if (out_fold_ms) out_fold_ms[round] = folded ? std::chrono::duration<float, std::milli>(t_end - t_fold).count() : 0.0f;
    if (out_round_ms) out_round_ms[round] = std::chrono::duration<float, std::milli>(t_end - t_round).count();
  }
  if (rc == PC_OK && n0 && have_u_prev) rc = pc_hip_te_ipa_key_scalars(ctx, curve, nullptr, 0, s_dev, n0, u_prev, 2, nullptr, nullptr);      // the last fold (size 2)
  if (rc == PC_OK) rc = n0 ? pc_hip_te_msm(ctx, srs, 0, s_dev, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n0, out_final_key_xy, nullptr)              // sum_j s_j K0_j
                           : pc_hip_te_srs_read(ctx, srs, 0, 1, out_final_key_xy);
  if (rc == PC_OK) rc = pc_hip_memcpy_d2h(ctx, out_c_host, coeffs_dev, TE_FR_BYTES);
  return rc;
}

}  // extern "C"
