// C ABI of the gfx950 backend (include/pc_hip.h): InnerProductArgPC::open over ed_on_bls12_381 (JubJub) on the device -- the vector
// kernels of the halving rounds over the curve's 252-bit scalar field, and the rounds as one call (ipa_pc/mod.rs:664-711).
// With them the two vector kernels of HyraxPC::open over that field, fr_lincomb and fr_dot (hyrax/mod.rs:347,356,391).
// This unit instantiates the FrVecOps part of FieldOpsImpl for that field (vec_table(): what the rounds and Hyrax need) and no other
// member: its 2-adicity is 1, there is no NTT over it (and no FieldOps table: pc_curve keeps its four ids).  The entry points over the
// table are abi_fr.hpp's, shared with the pc_curve fields.  The group side is abi_te.hip's, through the C ABI.
#include <chrono>
#include <string.h>
#include "abi_fr.hpp"
#include "abi_te.hpp"
#include "field_ops_impl.hpp"

namespace pc {
const FrVecOps& fr_vec_ops_ed_on_bls12_381() { static const FrVecOps t = FieldOpsImpl<TeFrP>::vec_table(); return t; }
}  // namespace pc

using pc::TE_POINT_BYTES;
using pc::TE_FR_BYTES;
typedef pc::host64::F64<pc::TeFrP> TeFr64;

extern "C" {

int pc_hip_te_fr_powers(pc_ctx* ctx, pc_te_curve curve, const void* z_host, size_t n, void* out_dev) {
  if (int rc = te_curve_check(curve)) return rc;
  return fr_powers_call(ctx, pc::fr_vec_ops_ed_on_bls12_381(), z_host, n, out_dev);
}

// <a, b> and sum_j xi[j] * polys[j] over the curve's scalar field: HyraxPC::open's <lt, r> and t.row_mul(l) (hyrax/mod.rs:347,356,391)
int pc_hip_te_fr_dot(pc_ctx* ctx, pc_te_curve curve, const void* a_dev, const void* b_dev, size_t n, void* out_host) {
  if (int rc = te_curve_check(curve)) return rc;
  return fr_dot_call(ctx, pc::fr_vec_ops_ed_on_bls12_381(), a_dev, b_dev, n, out_host);
}

int pc_hip_te_fr_lincomb(pc_ctx* ctx, pc_te_curve curve, const void* const* polys, pc_mem where_in, const size_t* lens,
                         size_t k, const void* xi_host, void* out, pc_mem where_out, size_t n_out) {
  if (int rc = te_curve_check(curve)) return rc;
  return fr_lincomb_call(ctx, pc::fr_vec_ops_ed_on_bls12_381(), polys, where_in, lens, k, xi_host, out, where_out, n_out);
}

int pc_hip_te_ipa_fold_dots(pc_ctx* ctx, pc_te_curve curve, void* coeffs_dev, void* z_dev, size_t m, const void* u_host, const void* u_inv_host,
                            void* out_dots_host) {
  if (int rc = te_curve_check(curve)) return rc;
  return ipa_fold_dots_call(ctx, pc::fr_vec_ops_ed_on_bls12_381(), coeffs_dev, z_dev, m, u_host, u_inv_host, out_dots_host);
}

int pc_hip_te_ipa_key_scalars(pc_ctx* ctx, pc_te_curve curve, const void* coeffs_dev, size_t m, void* s_dev, size_t n0,
                              const void* fold_u_host, size_t fold_m, void* out_l_dev, void* out_r_dev) {
  if (int rc = te_curve_check(curve)) return rc;
  return ipa_key_scalars_call(ctx, pc::fr_vec_ops_ed_on_bls12_381(), coeffs_dev, m, s_dev, n0, fold_u_host, fold_m, out_l_dev, out_r_dev);
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
