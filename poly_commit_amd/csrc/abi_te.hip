// C ABI of the gfx950 backend (include/pc_hip.h): the twisted Edwards curve ed_on_bls12_381 (JubJub) -- typed keys, the MSM and the key
// fold of InnerProductArgPC over it (ipa_pc/mod.rs:54-72, 699-707), and the many-MSM pass of HyraxPC::commit over a window table of a
// key range (hyrax/mod.rs:233-242).  This unit also instantiates everything templated on TeOf<T>
// (te.hpp, MsmPlan<TeOf<T>, HipBackend> with the digit and sort stages of its scalar field), and nothing of a short Weierstrass group.
#include <vector>
#include "abi_te.hpp"
#include "blocking_lane.hpp"

namespace pc {
namespace {

// The window table of the m resident points at b0 (te.hpp) on the context's queue, the doubled rows staged in its workspace.  Returns
// with the queue drained.
void te_window_table_sync(HipBackend& be, const uint32_t* b0, size_t m, uint32_t c, uint32_t Wd, uint32_t* table) {
  const TeNormBuf ws = te_norm_buf(be, m);
  te_window_table<TeC>(be, b0, m, c, Wd, table, ws.ext, ws.scratch, TE_NORM_K);
  be.sync();
}

// the key's own pipeline: the table-free single MSM, created on first use
BlockingLane* te_lane(pc_te_srs* k) {
  if (k->lane) return k->lane;
  MsmConfig cfg = k->ctx->msm_cfg;
  cfg.tbl = nullptr; cfg.tbl_c = 0;
  return k->lane = blocking_lane<TeC>(k->n, cfg, 0);
}

// the call's MSM on lane L, then what pc_hip_last_msm_shape and pc_hip_last_msm_phases_ms read
void te_run(pc_ctx* ctx, BlockingLane* L, const uint32_t* bases, uint32_t base_off, const void* scalars, pc_mem where, size_t n, pc_scalar_form form,
            uint32_t* out) {
  L->be.timing = ctx->be.timing;
  L->runner->run(bases, base_off, scalars, where, n, form == PC_SCALARS_MONTGOMERY, out);
  lane_phases(ctx, L);
}

void write_identity(uint32_t* out_xy) {
  for (int i = 0; i < TE_FQ_W; i++) { out_xy[i] = 0; out_xy[TE_FQ_W + i] = TeC::FqP::ONE[i]; }
}

}  // namespace
}  // namespace pc

using pc::TeC;
using pc::TE_AW;
using pc::TE_XY;
using pc::TE_POINT_BYTES;

extern "C" {

int pc_hip_te_srs_upload(pc_ctx* ctx, pc_te_curve curve, const void* bases, size_t n, size_t stride_bytes, pc_mem where, pc_te_srs** out) {
  if (!ctx || !out || (!bases && n)) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  if (where != PC_MEM_HOST && where != PC_MEM_DEVICE) return PC_ERR_INVALID_ARG;
  if (stride_bytes == 0) stride_bytes = TE_POINT_BYTES;
  if (stride_bytes < TE_POINT_BYTES) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  if (where == PC_MEM_DEVICE && stride_bytes != TE_POINT_BYTES) return PC_ERR_UNSUPPORTED;
  return key_make(ctx, out, [&]() { return te_key_create(ctx, curve, n, (size_t)TE_AW * 4); }, te_key_free, [&](pc_te_srs* k) {
    if (!n) return (int)PC_OK;
    // the caller's points, packed (twisted_edwards::Affine has no flag behind its coordinates: a larger stride is only skipped)
    std::vector<uint8_t> packed;
    const void* src = bases;
    if (where == PC_MEM_HOST && stride_bytes != TE_POINT_BYTES) {
      packed.resize(n * TE_POINT_BYTES);
      for (size_t i = 0; i < n; i++) memcpy(&packed[i * TE_POINT_BYTES], (const uint8_t*)bases + i * stride_bytes, TE_POINT_BYTES);
      src = packed.data();
    }
    Staged xy(ctx->be, src, where, n * TE_POINT_BYTES, true, 0);
    pc::TeDeriveBody<TeC> b{(const uint32_t*)xy.dev, k->bases};      // x || y -> x || y || 2 d x y
    ctx->be.launch(b, n);
    ctx->be.sync();
    return (int)PC_OK;
  });
}

void pc_hip_te_srs_free(pc_te_srs* k) { key_free_locked(k, te_key_free); }

size_t pc_hip_te_srs_len(const pc_te_srs* k) { return k ? k->n : 0; }

int pc_hip_te_srs_bytes_resident(const pc_te_srs* k, size_t out[4]) {
  if (!k || !out) return PC_ERR_INVALID_ARG;
  if (!k->ctx) { out[0] = out[1] = out[2] = out[3] = 0; return PC_OK; }
  std::lock_guard<std::recursive_mutex> lk(k->ctx->mu);
  te_key_bytes(k, out);
  return PC_OK;
}

int pc_hip_te_srs_read(pc_ctx* ctx, const pc_te_srs* k, size_t offset, size_t count, void* out_host) {
  if (!ctx || !k || k->ctx != ctx || offset > k->n || count > k->n - offset || (count && !out_host)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!count) return (int)PC_OK;
    CallBuf xy(ctx->be, 1, count * TE_POINT_BYTES);
    pc::TeStripBody<TeC> b{k->bases + offset * (size_t)TE_AW, (uint32_t*)xy.dev};
    ctx->be.launch(b, count);
    ctx->be.copy_d2h(out_host, xy.dev, count * TE_POINT_BYTES);
    return (int)PC_OK;
  });
}

int pc_hip_te_msm(pc_ctx* ctx, const pc_te_srs* kc, size_t base_offset, const void* scalars, pc_scalar_form form, pc_mem where, size_t n,
                  void* out_xy, int* out_is_identity) {
  pc_te_srs* k = const_cast<pc_te_srs*>(kc);
  if (!ctx || !k || !out_xy || k->ctx != ctx || base_offset > k->n) return PC_ERR_INVALID_ARG;
  if (where != PC_MEM_HOST && where != PC_MEM_DEVICE) return PC_ERR_INVALID_ARG;
  if (form != PC_SCALARS_CANONICAL && form != PC_SCALARS_MONTGOMERY) return PC_ERR_INVALID_ARG;
  const size_t avail = k->n - base_offset;      // msm_bigint semantics: min(bases.len(), scalars.len()) pairs
  if (n > avail) n = avail;
  if (n && !scalars) return PC_ERR_INVALID_ARG;
  if (!n) {                                      // the empty sum: the identity, no device work
    pc::write_identity((uint32_t*)out_xy);
    if (out_is_identity) *out_is_identity = 1;
    return PC_OK;
  }
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    pc::te_run(ctx, pc::te_lane(k), k->bases, (uint32_t)base_offset, scalars, where, n, form, (uint32_t*)out_xy);
    if (out_is_identity) *out_is_identity = pc::host64::te_is_identity<pc_te_ed_on_bls12_381>((const uint32_t*)out_xy) ? 1 : 0;
    return (int)PC_OK;
  });
}

int pc_hip_te_msm_many(pc_ctx* ctx, pc_te_srs* k, size_t base_offset, const void* scalars, pc_scalar_form form, pc_mem where,
                       size_t m, size_t n_msms, void* out_xy, int* out_is_identity) {
  if (!ctx || !k || k->ctx != ctx || !out_xy || (m && n_msms && !scalars)) return PC_ERR_INVALID_ARG;
  if (base_offset > k->n || m > k->n - base_offset) return PC_ERR_INVALID_ARG;
  if (where != PC_MEM_HOST && where != PC_MEM_DEVICE) return PC_ERR_INVALID_ARG;
  if (form != PC_SCALARS_CANONICAL && form != PC_SCALARS_MONTGOMERY) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!n_msms) return (int)PC_OK;
    uint32_t* out = (uint32_t*)out_xy;
    if (!m) {                                      // empty sums: identities, no device work
      for (size_t i = 0; i < n_msms; i++) { pc::write_identity(out + i * (size_t)TE_XY); if (out_is_identity) out_is_identity[i] = 1; }
      return (int)PC_OK;
    }
    const uint32_t c = pc::msm_choose_table_c(m, pc::TeFrP::BITS, 0), Wd = pc::msm_num_windows(pc::TeFrP::BITS, c);
    if ((uint64_t)n_msms * m * Wd >= (1ull << 31) || ((uint64_t)n_msms << (c - 1)) >= (1ull << 31)) return (int)PC_ERR_TOO_LARGE;
    pc_te_srs::Many& M = k->many;
    if (!M.lane || M.base_offset != base_offset || M.m != m || M.B != n_msms) {
      te_drop_many(k);
      const size_t bytes = (size_t)Wd * m * (size_t)TE_AW * 4;
      uint32_t* table = (uint32_t*)ctx->be.alloc(bytes);
      BlockingLane* L = nullptr;
      try {
        pc::te_window_table_sync(ctx->be, k->bases + base_offset * (size_t)TE_AW, m, c, Wd, table);
        pc::MsmConfig cfg = ctx->msm_cfg;
        cfg.c = 0; cfg.T = 0; cfg.tbl = table; cfg.tbl_c = c; cfg.tbl_stride = (uint32_t)m; cfg.tbl_pt_stride = (uint32_t)TE_AW; cfg.tbl_min_n = 0;
        cfg.tbl_glv = false;
        L = pc::blocking_lane<TeC>(n_msms * m, cfg, (uint32_t)n_msms);
      } catch (...) { (void)hipStreamSynchronize(ctx->be.stream); ctx->be.free(table); throw; }
      M.table = table; M.table_bytes = bytes; M.lane = L; M.base_offset = base_offset; M.m = m; M.B = n_msms;
    }
    pc::te_run(ctx, M.lane, k->bases, 0, scalars, where, n_msms * m, form, out);
    if (out_is_identity)
      for (size_t i = 0; i < n_msms; i++) out_is_identity[i] = pc::host64::te_is_identity<pc_te_ed_on_bls12_381>(out + i * (size_t)TE_XY) ? 1 : 0;
    return (int)PC_OK;
  });
}

int pc_hip_te_ec_fold(pc_ctx* ctx, pc_te_srs* k, size_t n_half, const void* u_host) {
  if (!ctx || !k || k->ctx != ctx || !u_host || 2 * n_half > k->n) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!n_half) return (int)PC_OK;
    pc::HipBackend& be = ctx->be;
    te_drop_fold_table(k);       // the key changes: its fold table is stale, and what was known about its points
    te_drop_many(k);             // ... and the window table of its many-MSM pass
    k->in_subgroup = -1;
    // the sums in extended coordinates, then the prefix products of the normalisation
    const pc::TeNormBuf ws = pc::te_norm_buf(be, n_half);
    pc::TeEcFoldBody<TeC> f;
    f.key = k->bases; f.half = (uint32_t)n_half; f.ext = ws.ext;
    const pc::Fd<pc::TeFrP> u = pc::Fd<pc::TeFrP>::load((const uint32_t*)u_host).from_mont();
    f.naf.from_scalar(u.l);
    be.launch(f, n_half);
    pc::te_normalise(be, ws.ext, ws.scratch, k->bases, n_half);
    be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_te_ec_fold_from(pc_ctx* ctx, const pc_te_srs* src, size_t n_half, const void* u_host, pc_te_srs** out) {
  if (!ctx || !src || src->ctx != ctx || !u_host || !out || !n_half || 2 * n_half > src->n) return PC_ERR_INVALID_ARG;
  return key_make(ctx, out, [&]() { return te_key_create(ctx, src->te_curve, n_half, (size_t)TE_AW * 4); }, te_key_free, [&](pc_te_srs* dst) {
    pc::HipBackend& be = ctx->be;
    const pc::TeNormBuf ws = pc::te_norm_buf(be, n_half);
    pc::NafMasks<pc::TE_FR_W> naf;
    naf.from_scalar(pc::Fd<pc::TeFrP>::load((const uint32_t*)u_host).from_mont().l);
    // from the key's table when it has one for this half and every digit of u has a row; the ladder otherwise: the same points
    pc::TeTableFoldBody<TeC> t;
    if (src->fold_tbl && 2 * n_half == src->n && t.dg.from_naf(naf, src->fold_rows)) {
      t.key = src->bases; t.tbl = src->fold_tbl; t.half = (uint32_t)n_half; t.ext = ws.ext;
      be.launch(t, n_half);
    } else {
      pc::TeEcFoldBody<TeC> f;
      f.key = src->bases; f.half = (uint32_t)n_half; f.ext = ws.ext; f.naf = naf;
      be.launch(f, n_half);
    }
    pc::te_normalise(be, ws.ext, ws.scratch, dst->bases, n_half);
    be.sync();
    if (src->in_subgroup == 1) dst->in_subgroup = 1;      // sums of multiples of subgroup points
    return (int)PC_OK;
  });
}

int pc_hip_te_srs_precompute_fold(pc_ctx* ctx, pc_te_srs* k) {
  if (!ctx || !k || k->ctx != ctx || k->n < 2 || (k->n & 1)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    te_drop_fold_table(k);
    pc::HipBackend& be = ctx->be;
    const size_t half = k->n / 2, row_words = half * (size_t)TE_AW, need = (size_t)pc::TE_FOLD_ROWS * row_words * 4;
    // refused above the share of the device's FREE memory that pc_hip_srs_precompute_fold allows (the same knob); folds then run the ladder
    static const double frac = []() { const char* e = getenv("PC_HIP_FOLD_TABLE_MAX_FRAC"); double v = e ? atof(e) : 0.5; return v < 0 ? 0.0 : v > 1 ? 1.0 : v; }();
    size_t free_b = 0, total_b = 0;
    PC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if ((double)need > frac * (double)free_b) {
      ctx->last_error = "fold table of " + std::to_string(need >> 20) + " MiB exceeds the allowed share of the free device memory";
      return (int)PC_ERR_UNSUPPORTED;
    }
    const pc::TeNormBuf ws = pc::te_norm_buf(be, half);
    uint32_t* tbl = (uint32_t*)be.alloc(need);
    try {
      be.copy_d2d(tbl, k->bases + row_words, row_words * 4);      // row 0: the upper half as it is
      for (uint32_t b = 0; b + 1 < pc::TE_FOLD_ROWS; b++) {     // row b + 1: one batched doubling of row b, normalised
        pc::TeDblRowBody<TeC> d{tbl + b * row_words, ws.ext};
        be.launch(d, half);
        pc::te_normalise(be, ws.ext, ws.scratch, tbl + (b + 1) * row_words, half);
      }
      be.sync();
    } catch (...) { (void)hipStreamSynchronize(be.stream); be.free(tbl); throw; }
    k->fold_tbl = tbl; k->fold_rows = pc::TE_FOLD_ROWS;
    return (int)PC_OK;
  });
}

int pc_hip_te_srs_fold_table_info(const pc_te_srs* k, unsigned* out_rows) {
  if (!k || !out_rows) return PC_ERR_INVALID_ARG;
  *out_rows = k->fold_tbl ? k->fold_rows : 0;
  return PC_OK;
}

int pc_hip_te_srs_in_subgroup(pc_ctx* ctx, pc_te_srs* k, int* out) {
  if (!ctx || !k || k->ctx != ctx || !out) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (k->in_subgroup >= 0) { *out = k->in_subgroup; return PC_OK; }
  return guarded(ctx, [&]() {
    int all = 1;
    if (k->n) {
      CallBuf flags(ctx->be, 1, k->n * 4);
      pc::TeSubgroupBody<TeC> b;
      b.key = k->bases; b.flags = (uint32_t*)flags.dev;
      b.naf.from_scalar(pc::TeFrP::MOD);
      ctx->be.launch(b, k->n);
      std::vector<uint32_t> h(k->n);
      ctx->be.copy_d2h(h.data(), flags.dev, k->n * 4);
      for (uint32_t f : h) all &= (int)(f & 1u);
    }
    k->in_subgroup = all;
    *out = all;
    return (int)PC_OK;
  });
}

int pc_hip_te_points_sum(pc_te_curve curve, const void* points, size_t count, void* out_xy) {
  if (!out_xy || (count && !points)) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  pc::host64::points_sum<TeC>((const uint32_t*)points, count, (uint32_t*)out_xy);
  return PC_OK;
}

int pc_hip_te_point_mul(pc_te_curve curve, const void* point, const void* scalar_mont, void* out_xy) {
  if (!point || !scalar_mont || !out_xy) return PC_ERR_INVALID_ARG;
  if (int rc = te_curve_check(curve)) return rc;
  pc::host64::scalar_mul<TeC>((const uint32_t*)point, pc::Fd<pc::TeFrP>::load((const uint32_t*)scalar_mont).from_mont().l, (uint32_t*)out_xy);
  return PC_OK;
}

}  // extern "C"
