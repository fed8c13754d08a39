// C ABI of the gfx950 backend (include/pc_hip.h): IPA -- vector kernels, key folds, the opening loop.
#include <chrono>
#include <string.h>
#include "abi_fr.hpp"

extern "C" {

// ---- IPA round kernels --------------------------------------------------------------------
int pc_hip_fr_fold(pc_ctx* ctx, pc_curve field_of, void* lo_dev, const void* hi_dev, size_t n_half, const void* s_host) {
  if (!ctx || !pc_known_curve(field_of) || !s_host || (n_half && (!lo_dev || !hi_dev))) return PC_ERR_INVALID_ARG;
  if (n_half >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n_half) pc::field_ops(field_of).fr_fold(ctx->be, (uint32_t*)lo_dev, (const uint32_t*)hi_dev, n_half, (const uint32_t*)s_host);
    return (int)PC_OK;
  });
}
int pc_hip_fr_dot(pc_ctx* ctx, pc_curve field_of, const void* a_dev, const void* b_dev, size_t n, void* out_host) {
  if (!pc_known_curve(field_of)) return PC_ERR_INVALID_ARG;
  return fr_dot_call(ctx, pc::field_ops(field_of), a_dev, b_dev, n, out_host);
}
int pc_hip_ipa_fold_dots(pc_ctx* ctx, pc_curve field_of, void* coeffs_dev, void* z_dev, size_t m, const void* u_host, const void* u_inv_host,
                         void* out_dots_host) {
  if (!pc_known_curve(field_of)) return PC_ERR_INVALID_ARG;
  return ipa_fold_dots_call(ctx, pc::field_ops(field_of), coeffs_dev, z_dev, m, u_host, u_inv_host, out_dots_host);
}
int pc_hip_fr_powers(pc_ctx* ctx, pc_curve field_of, const void* z_host, size_t n, void* out_dev) {
  if (!pc_known_curve(field_of)) return PC_ERR_INVALID_ARG;
  return fr_powers_call(ctx, pc::field_ops(field_of), z_host, n, out_dev);
}
int pc_hip_ipa_key_scalars(pc_ctx* ctx, pc_curve field_of, const void* coeffs_dev, size_t m, void* s_dev, size_t n0,
                           const void* fold_u_host, size_t fold_m, void* out_l_dev, void* out_r_dev) {
  if (!pc_known_curve(field_of)) return PC_ERR_INVALID_ARG;
  return ipa_key_scalars_call(ctx, pc::field_ops(field_of), coeffs_dev, m, s_dev, n0, fold_u_host, fold_m, out_l_dev, out_r_dev);
}
int pc_hip_ec_fold(pc_ctx* ctx, pc_srs* srs, size_t n_half, const void* u_host) {
  if (!ctx || !srs || srs->ctx != ctx || !u_host || 2 * n_half > srs->n) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    key_drain(srs);                             // queued MSMs still read the old key
    if (!n_half) return (int)PC_OK;
    drop_table(srs);                            // the key changes: its window tables are stale
    drop_many(srs);
    drop_fold_table(srs);
    if (srs->in_subgroup != 1) srs->in_subgroup = -1;      // a 1 stays (sums of multiples of subgroup points); anything else is forgotten
    pc::curve_ops(srs->curve).ec_fold_to(ctx->be, srs->bases, srs->bases, n_half, (const uint32_t*)u_host, nullptr, 0);
    return (int)PC_OK;
  });
}

int pc_hip_ec_fold_from(pc_ctx* ctx, const pc_srs* src, size_t n_half, const void* u_host, pc_srs** out) {
  if (!ctx || !src || src->ctx != ctx || !u_host || !out || !n_half || 2 * n_half > src->n) return PC_ERR_INVALID_ARG;
  return key_fold_to_working(ctx, const_cast<pc_srs*>(src), n_half, out, [&](pc_srs* dst) {
    const uint32_t* tbl = (src->fold_tbl && src->fold_levels == 1 && src->fold_half == n_half) ? src->fold_tbl : nullptr;
    pc::curve_ops(src->curve).ec_fold_to(ctx->be, src->bases, dst->bases, n_half, (const uint32_t*)u_host, tbl, src->fold_w);
  });
}
int pc_hip_ec_fold2_from(pc_ctx* ctx, const pc_srs* src, size_t n_quarter, const void* u1_host, const void* u2_host, pc_srs** out) {
  if (!ctx || !src || src->ctx != ctx || !u1_host || !u2_host || !out || !n_quarter || 4 * n_quarter > src->n) return PC_ERR_INVALID_ARG;
  return key_fold_to_working(ctx, const_cast<pc_srs*>(src), n_quarter, out, [&](pc_srs* dst) {
    const bool have = src->fold_tbl && src->fold_levels == 2 && src->fold_half == n_quarter;
    const pc::CurveOps& ops = pc::curve_ops(src->curve);
    const size_t aw = (size_t)src->aw;
    bool done = false;
    if (have) {
      // terms in the order of the table's points: K[q .. 2q) by u2, K[2q .. 3q) by u1, K[3q .. 4q) by u1 u2
      uint32_t u12[8];
      ops.fr_mul((const uint32_t*)u1_host, (const uint32_t*)u2_host, u12);
      const uint32_t* us[3] = {(const uint32_t*)u2_host, (const uint32_t*)u1_host, u12};
      done = ops.ec_fold_table(ctx->be, src->bases, dst->bases, n_quarter, src->fold_pts, 3, us, src->fold_w, src->fold_tbl);
    }
    if (!done) {
      // no two-level table on this key (or a split beyond its rows): the two folds one after the other, through a scratch half key
      uint32_t* tmp = (uint32_t*)ctx->be.alloc(2 * n_quarter * aw * 4);
      try {
        const uint32_t* tbl1 = (src->fold_tbl && src->fold_levels == 1 && src->fold_half == 2 * n_quarter) ? src->fold_tbl : nullptr;
        ops.ec_fold_to(ctx->be, src->bases, tmp, 2 * n_quarter, (const uint32_t*)u1_host, tbl1, src->fold_w);
        ops.ec_fold_to(ctx->be, tmp, tmp, n_quarter, (const uint32_t*)u2_host, nullptr, 2);
        ctx->be.copy_d2d(dst->bases, tmp, n_quarter * aw * 4);
        ctx->be.sync();
      } catch (...) { ctx->be.free(tmp); throw; }
      ctx->be.free(tmp);
    }
  });
}

int pc_hip_ipa_round2_msms(pc_ctx* ctx, const pc_srs* srs_c, const void* coeffs_dev, size_t n_quarter, const void* u1_host,
                           void* out_l_xy, int* out_l_is_infinity, void* out_r_xy, int* out_r_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || srs->ctx != ctx || !coeffs_dev || !u1_host || !out_l_xy || !out_r_xy || !n_quarter || 4 * n_quarter > srs->n) return PC_ERR_INVALID_ARG;
  if (3 * n_quarter >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const size_t q = n_quarter, fw = 8;                                    // scalars: 8 words each
    const size_t bytes = 2 * 3 * q * fw * 4;
    // scalar vectors (c_r | 0 | u1 c_r) and (c_l | 0 | u1 c_l): the context's grow-only call buffer up to STAGE_KEEP, transient above it
    CallBuf call_buf(ctx->be, 0, bytes);
    uint32_t* buf = (uint32_t*)call_buf.dev;
    uint32_t* sl = buf; uint32_t* sr = buf + 3 * q * fw;
    const uint32_t* c = (const uint32_t*)coeffs_dev;
    ctx->be.memset(buf, 0, bytes);
    ctx->be.copy_d2d(sl, c + q * fw, q * fw * 4);                          // c_r = coeffs[q .. 2q)
    ctx->be.copy_d2d(sr, c, q * fw * 4);                                   // c_l = coeffs[0 .. q)
    const pc::FieldOps& fo = pc::field_ops(srs->curve);
    fo.fr_fold(ctx->be, sl + 2 * q * fw, c + q * fw, q, (const uint32_t*)u1_host);      // 0 + u1 c_r
    fo.fr_fold(ctx->be, sr + 2 * q * fw, c, q, (const uint32_t*)u1_host);               // 0 + u1 c_l
    ctx->be.sync();                                                        // the pipelines run on queues of their own
    StackJob jl(ctx), jr(ctx);
    int rc = enqueue_job(ctx, srs, 0, sl, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, 3 * q, out_l_xy, out_l_is_infinity, &jl.job);
    if (rc != PC_OK) return rc;
    rc = enqueue_job(ctx, srs, q, sr, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, 3 * q, out_r_xy, out_r_is_infinity, &jr.job);
    if (rc != PC_OK) return rc;
    if (!jl.job.done) complete_job(ctx, &jl.job);
    if (!jr.job.done) complete_job(ctx, &jr.job);
    return jl.job.status != PC_OK ? jl.job.status : jr.job.status;
  });
}

// The halving loop of InnerProductArgPC::open (ipa_pc/mod.rs:664-711) as ONE call: everything the round-by-round entry points above do,
// in the order poly_commit_amd/ipa.py and host/ipa_pc.hpp drive them, without a host language between the rounds (measured: 61.1-61.9 ms
// against 62.2 ms driven from Python at 2^22 -- the rounds are bound by the device's dependency chain; what the call buys a binding is
// one entry point instead of ~150 calls).  The transcript stays the caller's: `next_challenge`
// gets the round's l and r (affine, Montgomery x || y; all zeros = infinity) and returns the challenge u (Montgomery Fr).
static bool ipa_fixed_table() {      // PC_HIP_IPA_FIXED_TABLE=0: the late rounds run table-free on the working key (round 5's form)
  static const bool on = []() { const char* e = getenv("PC_HIP_IPA_FIXED_TABLE"); return !(e && !strcmp(e, "0")); }();
  return on;
}
int pc_hip_ipa_open_rounds(pc_ctx* ctx, const pc_srs* comm_key, void* coeffs_dev, size_t n, const void* point_host, const void* h_prime_xy_host,
                           pc_ipa_challenge_fn next_challenge, void* user, size_t fixed_key_below,
                           void* out_l_vec_xy, void* out_r_vec_xy, void* out_final_key_xy, void* out_c_host, float* out_round_ms, float* out_fold_ms) {
  pc_srs* root = const_cast<pc_srs*>(comm_key);
  if (!ctx || !root || root->ctx != ctx || !coeffs_dev || !n || (n & (n - 1)) || n > root->n || !point_host || !h_prime_xy_host || !next_challenge ||
      !out_final_key_xy || !out_c_host || (n > 1 && (!out_l_vec_xy || !out_r_vec_xy))) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  const pc_curve curve = root->curve;
  const pc::CurveOps& ops = pc::curve_ops(curve);
  const size_t pb = (size_t)root->aw * 4;                       // bytes of an affine point
  // the default: 2^17 when the fixed key gets its window table (56.6 ms at 2^22 against 57.5 with 2^16 and 62.2 with 2^18), 2^16 without
  // one (EXPERIMENTS 00); any value below 2: the key is folded in every round
  if (!fixed_key_below) fixed_key_below = (size_t)1 << (ipa_fixed_table() ? 17 : 16);
  pc_srs* srs = root; bool owned = false;
  pc_srs* fixed = nullptr;                                      // the fixed key's own object (window table), or null: the working key serves the late rounds
  struct KeyGuard { pc_srs*& k; bool& owned; ~KeyGuard() { if (owned && k) pc_hip_srs_free(k); } } key_guard{srs, owned};
  void* z = nullptr; void* s_dev = nullptr; char* alr = nullptr;
  int rc = guarded(ctx, [&]() { z = ipa_buffer(ctx, 0, n * 32); return (int)PC_OK; });
  if (rc != PC_OK) return rc;
  char* c = (char*)coeffs_dev;
  rc = pc_hip_fr_powers(ctx, curve, point_host, n, z);                                          // z = (1, point, point^2, ..)   :641-649
  uint32_t dots[2][8];
  if (rc == PC_OK) rc = pc_hip_ipa_fold_dots(ctx, curve, c, z, n, nullptr, nullptr, dots);      // the inner products of the first round
  size_t n0 = 0;
  uint32_t u_prev[8], u_first[8], u[8], ui[8], one[8];
  bool have_u_prev = false, have_u_first = false;
  ops.fr_one(one);
  // a committer key with a two-level fold table (pc_hip_srs_precompute_fold_ex): round 1 leaves the key alone, round 2 runs on it by
  // linearity (pc_hip_ipa_round2_msms), the key after both folds comes out of the table in one step (pc_hip_ec_fold2_from)
  bool two_level = n == root->n && n >= 8 && n / 2 > fixed_key_below && root->fold_tbl && root->fold_levels == 2;
  std::vector<uint32_t> pts(4 * (size_t)root->aw);               // ml | hl | mr | hr
  size_t round = 0;
  using clk = std::chrono::steady_clock;
  for (size_t m = n; rc == PC_OK && m > 1; m /= 2, round++) {
    const auto t_round = clk::now();
    const size_t h = m / 2;
    if (!n0 && m <= fixed_key_below) {                                                          // from here on key[0 .. n0) stays fixed
      n0 = m;
      rc = guarded(ctx, [&]() { s_dev = ipa_buffer(ctx, 1, n0 * 32); alr = (char*)ipa_buffer(ctx, 2, 2 * n0 * 32); return (int)PC_OK; });
      if (rc == PC_OK) rc = pc_hip_fr_powers(ctx, curve, one, n0, s_dev);                        // s = (1, 1, ..)
      if (rc != PC_OK) break;
      have_u_prev = false;                                                                      // the key itself carries every fold so far
      if (ipa_fixed_table() && srs == root && root->table && n0 >= root->cfg.tbl_min_n) {
        fixed = root;                                                                           // no fold yet and the committer key has its window table: it IS the fixed key, nothing to copy or refill
      } else if (ipa_fixed_table() && n0 >= ((size_t)1 << 12) && n0 <= ((size_t)1 << 18)) {
        fixed = key_fixed(ctx, root, srs, n0);                                                  // (on any failure the rounds run table-free on the working key, as before)
      }
    }
    uint32_t* ml = pts.data(); uint32_t* hl = ml + root->aw; uint32_t* mr = hl + root->aw; uint32_t* hr = mr + root->aw;
    pc_job* jl = nullptr; pc_job* jr = nullptr;
    // l = cm_commit(key_l, coeffs_r) + h' <coeffs_r, z_l>;  r = cm_commit(key_r, coeffs_l) + h' <coeffs_l, z_r>          :666-675
    if (n0) {
      rc = pc_hip_ipa_key_scalars(ctx, curve, c, m, s_dev, n0, have_u_prev ? u_prev : nullptr, have_u_prev ? 2 * m : 0, alr, alr + 32 * n0);
      if (rc == PC_OK) rc = pc_hip_msm_async(ctx, fixed ? fixed : srs, 0, alr, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n0, ml, nullptr, &jl);
      if (rc == PC_OK) rc = pc_hip_msm_async(ctx, fixed ? fixed : srs, 0, alr + 32 * n0, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n0, mr, nullptr, &jr);
    } else if (have_u_first) {
      rc = pc_hip_ipa_round2_msms(ctx, srs, c, h, u_first, ml, nullptr, mr, nullptr);
    } else {
      rc = pc_hip_msm_async(ctx, srs, 0, c + 32 * h, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, h, ml, nullptr, &jl);
      if (rc == PC_OK) rc = pc_hip_msm_async(ctx, srs, h, c, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, h, mr, nullptr, &jr);
    }
    if (rc == PC_OK) {                                                                          // beside the MSMs: h' * <.., ..>, one point each
      ops.point_mul((const uint32_t*)h_prime_xy_host, dots[0], hl);
      ops.point_mul((const uint32_t*)h_prime_xy_host, dots[1], hr);
    }
    const int w1 = jl ? pc_hip_job_wait(ctx, jl) : PC_OK, w2 = jr ? pc_hip_job_wait(ctx, jr) : PC_OK;      // always reap queued jobs
    if (rc == PC_OK) rc = w1 != PC_OK ? w1 : w2;
    if (rc != PC_OK) break;
    uint32_t* l = (uint32_t*)((char*)out_l_vec_xy + round * pb); uint32_t* r = (uint32_t*)((char*)out_r_vec_xy + round * pb);
    ops.points_sum(ml, 2, l);
    ops.points_sum(mr, 2, r);
    next_challenge(user, l, r, u);                                                              // :681-689, the caller's transcript
    ops.fr_inv(u, ui);
    rc = pc_hip_ipa_fold_dots(ctx, curve, c, z, h, u, ui, dots);                                // :691-697 + the next round's inner products
    if (rc != PC_OK) break;
    const auto t_fold = clk::now();
    bool folded = false;
    if (n0) { memcpy(u_prev, u, 32); have_u_prev = true; }                                      // applied to the factors at the top of the next round
    else if (two_level && !have_u_first && srs == root) { memcpy(u_first, u, 32); have_u_first = true; }
    else if (have_u_first) {
      pc_srs* work = nullptr;
      rc = pc_hip_ec_fold2_from(ctx, root, h, u_first, u, &work);
      if (rc == PC_OK) { srs = work; owned = true; }
      have_u_first = false; two_level = false; folded = true;
    } else if (owned) { rc = pc_hip_ec_fold(ctx, srs, h, u); folded = true; }                   // key_l += u key_r, normalised          :699-707
    else {
      pc_srs* work = nullptr;
      rc = pc_hip_ec_fold_from(ctx, srs, h, u, &work);                                          // the same fold, out of place: the committer key stays
      if (rc == PC_OK) { srs = work; owned = true; }
      folded = true;
    }
    const auto t_end = clk::now();
    if (out_fold_ms) out_fold_ms[round] = folded ? std::chrono::duration<float, std::milli>(t_end - t_fold).count() : 0.0f;
    if (out_round_ms) out_round_ms[round] = std::chrono::duration<float, std::milli>(t_end - t_round).count();
  }
  if (rc == PC_OK && n0 && have_u_prev) rc = pc_hip_ipa_key_scalars(ctx, curve, nullptr, 0, s_dev, n0, u_prev, 2, nullptr, nullptr);      // the last fold (size 2)
  if (rc == PC_OK) rc = n0 ? pc_hip_msm(ctx, fixed ? fixed : srs, 0, s_dev, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, n0, out_final_key_xy, nullptr)           // sum_j s_j K0_j
                           : pc_hip_srs_read(ctx, srs, 0, 1, out_final_key_xy);
  if (rc == PC_OK) rc = pc_hip_memcpy_d2h(ctx, out_c_host, coeffs_dev, 32);
  return rc;
}

int pc_hip_point_mul(pc_curve curve, const void* point_xy, const void* scalar_mont, void* out_xy) {
  if (!pc_known_curve(curve) || !point_xy || !scalar_mont || !out_xy) return PC_ERR_INVALID_ARG;
  pc::curve_ops(curve).point_mul((const uint32_t*)point_xy, (const uint32_t*)scalar_mont, (uint32_t*)out_xy);
  return PC_OK;
}
int pc_hip_fixed_base_batch_mul(pc_ctx* ctx, pc_curve curve, const void* g_xy_host, const void* scalars_dev, size_t n,
                                void* out_points_dev) {
  if (!ctx || !pc_known_curve(curve) || !g_xy_host || (n && (!scalars_dev || !out_points_dev))) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!n) return (int)PC_OK;
    pc::curve_ops(curve).fixed_base(ctx->be, (const uint32_t*)g_xy_host, (const uint32_t*)scalars_dev, n, (uint32_t*)out_points_dev, pc::FIXED_BASE_K_KZG);
    return (int)PC_OK;
  });
}

}  // extern "C"
