// C ABI of the gfx950 backend (include/pc_hip.h): key upload, serialisation, window and fold tables, residency of one key.
#include <string.h>
#include "abi.hpp"

extern "C" {

int pc_hip_srs_upload(pc_ctx* ctx, pc_curve curve, const void* bases, size_t n, size_t stride_bytes, pc_mem where,
                      pc_srs** out) {
  if (!ctx || !out || (!bases && n) || !pc_known_curve(curve)) return PC_ERR_INVALID_ARG;
  const size_t pb = 2 * (size_t)fq_bytes(curve);
  if (stride_bytes == 0) stride_bytes = pb;
  if (stride_bytes < pb) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  if (where == PC_MEM_DEVICE && stride_bytes != pb) return PC_ERR_UNSUPPORTED;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  *out = nullptr;
  pc_srs* srs = nullptr;
  int rc = guarded(ctx, [&]() {
    srs = key_create(ctx, curve, n);
    if (!srs) return (int)PC_ERR_OOM;
    key_base_fill(srs, bases, n, stride_bytes, where);
    if (const char* e = getenv("PC_HIP_SEG_TAIL")) srs->cfg.seg_tail_lanes = (uint32_t)atoi(e);   // tuning experiments
    if (const char* e = getenv("PC_HIP_T2")) srs->cfg.T2 = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_T2B")) srs->cfg.T2b = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_K0")) srs->cfg.K0 = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_TBL_K0")) srs->cfg.tbl_K0 = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_TBL_LANES")) srs->cfg.tbl_target_lanes = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_TBL_CHUNK")) srs->cfg.tbl_chunk = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_TBL_MAX_LANES")) srs->cfg.tbl_max_lanes = (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_COOP_MAX_LOG2")) srs->cfg.coop_max_points = 1u << (uint32_t)atoi(e);
    if (const char* e = getenv("PC_HIP_COOP2_MAX_LOG2")) { int v = atoi(e); srs->cfg.coop2_max_points = v < 0 ? 0u : 1u << (uint32_t)(v > 30 ? 30 : v); }
    srs_lane(srs, 0);   // allocate the first pipeline now so that OOM surfaces at upload
    return (int)PC_OK;
  });
  if (rc != PC_OK) { if (srs) key_free(srs); return rc; }
  *out = srs;
  return PC_OK;
}

static size_t g1_point_bytes(pc_curve curve, int compressed) {
  const size_t fb = (size_t)fq_bytes(curve);
  const size_t bits = curve == PC_CURVE_BLS12_381 ? 381 : curve == PC_CURVE_BN254 ? 254 : curve == PC_CURVE_BLS12_377 ? 377 : 255;
  const size_t yb = (bits + 2 + 7) / 8;
  return curve == PC_CURVE_BLS12_381 ? (compressed ? fb : 2 * fb) : (compressed ? yb : fb + yb);
}

int pc_hip_srs_load_serialized(pc_ctx* ctx, pc_curve curve, const void* bytes, size_t n_bytes, int compressed, size_t max_points,
                               pc_srs** out, size_t* out_points, size_t* out_bytes_consumed) {
  if (!ctx || !out || !bytes || !pc_known_curve(curve)) return PC_ERR_INVALID_ARG;
  *out = nullptr;
  if (n_bytes < 8) return PC_ERR_INVALID_ARG;
  const size_t fb = (size_t)fq_bytes(curve), pbytes = g1_point_bytes(curve, compressed);
  uint64_t len = 0; memcpy(&len, bytes, 8);                                    // Vec<T>: u64 little-endian length
  if (len > (n_bytes - 8) / pbytes) return PC_ERR_INVALID_ARG;                 // truncated input
  const size_t n = max_points && max_points < len ? max_points : (size_t)len;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  void* raw = nullptr; void* pts = nullptr;
  uint32_t bad = 0;
  int rc = guarded(ctx, [&]() {
    raw = ctx->be.alloc(n * pbytes); pts = ctx->be.alloc((n ? n : 1) * 2 * fb);
    if (n) {
      ctx->be.copy_h2d(raw, (const char*)bytes + 8, n * pbytes);
      bad = pc::curve_ops(curve).srs_decode(ctx->be, (const uint8_t*)raw, n, compressed, (uint32_t*)pts);
    }
    return (int)PC_OK;
  });
  if (rc == PC_OK && bad) { ctx->last_error = std::to_string(bad) + " serialized point(s) are not on the curve"; rc = PC_ERR_INVALID_ARG; }
  if (rc == PC_OK) rc = pc_hip_srs_upload(ctx, curve, pts, n, 0, PC_MEM_DEVICE, out);
  (void)guarded(ctx, [&]() { ctx->be.free(raw); ctx->be.free(pts); return (int)PC_OK; });
  if (rc == PC_OK) { if (out_points) *out_points = n; if (out_bytes_consumed) *out_bytes_consumed = 8 + (size_t)len * pbytes; }
  return rc;
}

int pc_hip_srs_serialize(pc_ctx* ctx, const pc_srs* srs, size_t offset, size_t count, int compressed, void* out_bytes_host, size_t capacity,
                         size_t* out_written) {
  if (!ctx || !srs || srs->ctx != ctx || offset > srs->n || count > srs->n - offset || !out_written) return PC_ERR_INVALID_ARG;
  const size_t pbytes = g1_point_bytes(srs->curve, compressed), need = 8 + count * pbytes;
  *out_written = need;
  if (!out_bytes_host || capacity < need) return out_bytes_host ? PC_ERR_INVALID_ARG : PC_OK;      // NULL buffer: size query
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const uint64_t len = count;
    memcpy(out_bytes_host, &len, 8);                                                                // Vec<T>: u64 little-endian length
    if (!count) return (int)PC_OK;
    void* dev = ctx->be.alloc(count * pbytes);
    try {
      pc::curve_ops(srs->curve).srs_encode(ctx->be, srs->bases + offset * (size_t)srs->aw, count, compressed, (uint8_t*)dev);
      ctx->be.copy_d2h((char*)out_bytes_host + 8, dev, count * pbytes);
    } catch (...) { ctx->be.free(dev); throw; }
    ctx->be.free(dev);
    return (int)PC_OK;
  });
}

int pc_hip_universal_params_layout(pc_curve curve, const void* bytes, size_t n_bytes, int compressed, size_t out[9]) {
  // kzg10::UniversalParams, CanonicalSerialize order (kzg10/data_structures.rs:57-77):
  //   powers_of_g: Vec<G1Affine> | powers_of_gamma_g: BTreeMap<usize, G1Affine> | h: G2Affine | beta_h: G2Affine |
  //   neg_powers_of_h: BTreeMap<usize, G2Affine>        (Vec / BTreeMap: u64 LE length first; map entries: u64 LE key, value)
  if (!bytes || !out || ((int)curve != PC_CURVE_BLS12_381 && (int)curve != PC_CURVE_BN254 && (int)curve != PC_CURVE_BLS12_377)) return PC_ERR_INVALID_ARG;   // pairing curves only
  const size_t g1 = g1_point_bytes(curve, compressed);
  // G2 over Fq2: BLS12-381 (zcash): 96 / 192 bytes; BN254 and BLS12-377 (generic SW over Fq2, flags in the spare bits of the last byte):
  // 64 / 128 and 96 / 192
  const size_t fb = (size_t)fq_bytes(curve), g2 = compressed ? 2 * fb : 4 * fb;
  const uint8_t* p = (const uint8_t*)bytes;
  size_t at = 0;
  auto take_len = [&](uint64_t& v) { if (n_bytes - at < 8) return false; memcpy(&v, p + at, 8); at += 8; return true; };
  uint64_t n_g = 0, n_gg = 0, n_neg = 0;
  out[0] = at; if (!take_len(n_g) || n_g > (n_bytes - at) / g1) return PC_ERR_INVALID_ARG;
  out[1] = (size_t)n_g; at += (size_t)n_g * g1;
  out[2] = at; if (!take_len(n_gg) || n_gg > (n_bytes - at) / (8 + g1)) return PC_ERR_INVALID_ARG;
  out[3] = (size_t)n_gg; at += (size_t)n_gg * (8 + g1);
  if (n_bytes - at < 2 * g2) return PC_ERR_INVALID_ARG;
  out[4] = at; at += g2;                                   // h
  out[5] = at; at += g2;                                   // beta_h
  out[6] = at; if (!take_len(n_neg) || n_neg > (n_bytes - at) / (8 + g2)) return PC_ERR_INVALID_ARG;
  out[7] = (size_t)n_neg; at += (size_t)n_neg * (8 + g2);
  out[8] = at;                                             // total size of the structure
  return PC_OK;
}

// Every path mutates shared context state (ctx->keys, the backend's byte ledger, a parent's work cache) and is reached from arbitrary
// threads (Drop of the last Arc<ResidentKey>, device::release, the LRU eviction of the Rust shim) while other threads may be inside
// pc_hip_srs_upload / pc_hip_ctx_trim / any alloc: the context lock is held for the whole call (recursive: pc_hip_ctx_trim and the
// work-cache recursion below re-enter).  The mutex lives in the context; pc_hip_shutdown releases every key still alive and leaves it with ctx == nullptr, so a key freed after its context never touches that mutex.
void pc_hip_srs_free(pc_srs* srs) { key_free_locked(srs, key_free); }
int pc_hip_srs_precompute_ex(pc_ctx* ctx, pc_srs* srs, unsigned window_bits, size_t min_pairs, unsigned flags) {
  if (!ctx || !srs || srs->ctx != ctx || window_bits == 1 || window_bits > 23 || (flags & ~(unsigned)(PC_HIP_TABLE_GLV | PC_HIP_TABLE_GLV_IF_TIGHT | PC_HIP_TABLE_GLV_IF_LARGE))) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    key_drain(srs);
    drop_table(srs);
    if (!srs->n) return (int)PC_OK;
    const uint32_t bits = pc::curve_ops(srs->curve).scalar_bits;
    // 96-byte points (BLS12-381) are padded to one 128-byte line each: a gather then touches one
    // DRAM line instead of 1.5 on average (the table no longer fits the 256 MB MALL)
    uint32_t pt_stride = srs->aw == 24 ? 32u : (uint32_t)srs->aw;
    if (const char* e = getenv("PC_HIP_TBL_PAD")) { if (!atoi(e)) pt_stride = (uint32_t)srs->aw; }      // =0: packed 96-byte rows
    bool glv = (flags & PC_HIP_TABLE_GLV) != 0;
    auto geometry = [&](bool g, uint32_t& c, uint32_t& Wt, size_t& bytes) {
      c = window_bits ? window_bits : pc::msm_choose_table_c(srs->n, bits, 5, g);
      if (const char* e = getenv("PC_HIP_TBL_C")) { if (!window_bits && atoi(e) >= 4 && atoi(e) <= 24) c = (uint32_t)atoi(e); }      // measurements only
      Wt = table_windows(srs, c, g);
      bytes = (size_t)Wt * srs->n * pt_stride * 4;
    };
    uint32_t c, Wt; size_t bytes;
    geometry(glv, c, Wt, bytes);
    if (!glv && (flags & PC_HIP_TABLE_GLV_IF_LARGE)) {
      // large keys: half the table (a 2^24-point BLS12-381 key: 12.9 instead of 25.8 GB) for one more bucket set to reduce; small keys
      // keep the full table (at 2^20 the second set's reduction costs 20 % of an MSM, the table only 1.6 GB)
      static const size_t large = []() { const char* e = getenv("PC_HIP_TABLE_GLV_LARGE_MB"); return (size_t)(e ? atol(e) : 4096) << 20; }();
      if (bytes > large) { glv = true; geometry(glv, c, Wt, bytes); }
    }
    if (!glv && (flags & PC_HIP_TABLE_GLV_IF_TIGHT)) {
      // the full table (bits / c + 1 copies of the key: 25.8 GB for 2^24 BLS12-381 points) only when it leaves half of the free
      // memory to everything else; otherwise the GLV form (half the windows: the same additions, one more bucket set to reduce)
      size_t free_b = 0, total_b = 0;
      PC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      if (bytes > free_b / 2) { glv = true; geometry(glv, c, Wt, bytes); }
    }
    if ((uint64_t)Wt * srs->n >= (1ull << 31)) return (int)PC_ERR_TOO_LARGE;     // entry = 31-bit table index + sign
    uint32_t* table = (uint32_t*)ctx->be.alloc(bytes);
    try {
      pc::curve_ops(srs->curve).window_table(ctx->be, srs->bases, (uint32_t)srs->n, c, Wt, table, pt_stride);
    } catch (...) { ctx->be.free(table); throw; }
    key_delete_lanes(srs);
    srs->table = table;
    srs->cfg.tbl = table; srs->cfg.tbl_c = c; srs->cfg.tbl_stride = (uint32_t)srs->n; srs->cfg.tbl_pt_stride = pt_stride; srs->cfg.tbl_glv = glv;
    srs->cfg.tbl_min_n = min_pairs ? min_pairs : (srs->n + 3) / 4;
    try { srs_lane(srs, 0); }                     // workspace for the table geometry; on failure fall back
    catch (...) { drop_table(srs); srs_lane(srs, 0); throw; }
    return (int)PC_OK;
  });
}
int pc_hip_srs_precompute(pc_ctx* ctx, pc_srs* srs, unsigned window_bits, size_t min_pairs) {
  // PC_HIP_TABLE_GLV=1: every table in the GLV form; =0: never; =large: for keys whose full table exceeds 4 GiB; unset: the full table
  // unless device memory is tight (round 5: the GLV form costs 7 % of a pipelined 2^24 step -- split 0.6 ms, second bucket set 1.1 ms --
  // for 12.9 GB less: speed is the default, memory the option)
  static const unsigned flags = []() { const char* e = getenv("PC_HIP_TABLE_GLV"); return !e ? (unsigned)PC_HIP_TABLE_GLV_IF_TIGHT : !strcmp(e, "large") ? (unsigned)(PC_HIP_TABLE_GLV_IF_TIGHT | PC_HIP_TABLE_GLV_IF_LARGE) : atoi(e) ? (unsigned)PC_HIP_TABLE_GLV : 0u; }();
  return pc_hip_srs_precompute_ex(ctx, srs, window_bits, min_pairs, flags);
}
size_t pc_hip_srs_len(const pc_srs* srs) { return srs ? srs->n : 0; }
void* pc_hip_srs_device_ptr(const pc_srs* srs) { return srs ? srs->bases : nullptr; }

int pc_hip_srs_bytes_resident(const pc_srs* srs, size_t out[4]) {
  if (!srs || !out) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(srs->ctx->mu);
  key_bytes(srs, out);
  return PC_OK;
}

int pc_hip_srs_precompute_fold_ex(pc_ctx* ctx, pc_srs* srs, unsigned levels, unsigned naf_width) {
  if (!ctx || !srs || srs->ctx != ctx || levels > 2 || (naf_width && (naf_width < 2 || naf_width > 5))) return PC_ERR_INVALID_ARG;
  if (srs->n < 2 || (srs->n & 1) || (levels == 2 && (srs->n & 3))) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    drop_fold_table(srs);
    const size_t pb = (size_t)srs->aw * 4;
    const pc::CurveOps& ops = pc::curve_ops(srs->curve);
    // Refused above a share of the device's FREE memory (PC_HIP_FOLD_TABLE_MAX_FRAC, default 0.5) instead of driving a shared GPU out
    // of memory; the opening then runs the GLV ladder.  levels / naf_width 0: the largest form that fits that share -- two levels
    // from 2^16 points on (below, the second fold is a latency-bound ladder either way), digits as wide as the memory allows:
    //   rows = 131 * 2^(w-2), points per row = n / 2 or 3 n / 4:  a 2^22-point Pallas key: 17.6 GB (1, 2) .. 26 / 53 / 106 GB (2, 2 / 3 / 4)
    static const double frac = []() { const char* e = getenv("PC_HIP_FOLD_TABLE_MAX_FRAC"); double v = e ? atof(e) : 0.5; return v < 0 ? 0.0 : v > 1 ? 1.0 : v; }();
    size_t free_b = 0, total_b = 0;
    PC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    auto bytes_of = [&](unsigned L, unsigned w) { return ((size_t)ops.fold_rows << (w - 2)) * (srs->n - (srs->n >> L)) * pb; };
    // the forms in the order of the opening times measured on a 2^22-point Pallas key (EXPERIMENTS 00): (2,4) 63.6 ms, (2,3) 66.8,
    // (1,4) 69.6, (2,2) 70.9, (1,3), (1,2) 73.7; the first one the caller's choice allows and the memory share holds
    static const unsigned order[6][2] = {{2, 4}, {2, 3}, {1, 4}, {2, 2}, {1, 3}, {1, 2}};
    const bool two_ok = srs->n >= ((size_t)1 << 16) && !(srs->n & 3);      // (below 2^16 points the second fold is a latency-bound ladder either way)
    unsigned L = 0, w = 0; size_t need = 0;
    for (const auto& f : order) {
      if (levels ? f[0] != levels : (f[0] == 2 && !two_ok)) continue;
      if (naf_width && f[1] != naf_width) continue;
      need = bytes_of(f[0], f[1]);
      if ((double)need <= frac * (double)free_b) { L = f[0]; w = f[1]; break; }
    }
    if (!L && naf_width == 5)      // width 5 (43 additions per term, twice the rows of width 4) only on request
      for (unsigned l : {2u, 1u}) {
        if (levels ? l != levels : (l == 2 && !two_ok)) continue;
        need = bytes_of(l, 5);
        if ((double)need <= frac * (double)free_b) { L = l; w = 5; break; }
      }
    if (!L) {
      ctx->last_error = "fold table of " + std::to_string(need >> 20) + " MiB exceeds " + std::to_string(frac) + " of the free device memory (" + std::to_string(free_b >> 20) + " MiB)";
      return (int)PC_ERR_UNSUPPORTED;
    }
    const size_t q = srs->n >> L, pts = srs->n - q;
    uint32_t* t = (uint32_t*)ctx->be.alloc(need);
    try { ops.fold_table_build(ctx->be, srs->bases + q * (size_t)srs->aw, pts, w, t); }
    catch (...) { ctx->be.free(t); throw; }
    srs->fold_tbl = t; srs->fold_half = q; srs->fold_pts = pts; srs->fold_levels = L; srs->fold_w = w;
    // The working key the first opening on this key will fold into (q points and three pipelines: ~10 ms of allocations) is made now,
    // with the table, instead of inside that opening; it waits in the key's cache like one an opening handed back (pc_hip_ctx_trim
    // releases it, pc_hip_ec_fold[2]_from re-creates it on demand).
    key_premake_working(ctx, srs, q);
    return (int)PC_OK;
  });
}
int pc_hip_srs_precompute_fold(pc_ctx* ctx, pc_srs* srs) {
  // PC_HIP_FOLD_TABLE="levels,width" (e.g. "1,2": the one-level table of plain NAF digits of rounds 3-5); unset: the library's choice
  static const std::pair<unsigned, unsigned> form = []() {
    const char* e = getenv("PC_HIP_FOLD_TABLE"); unsigned l = 0, w = 0;
    if (e) { l = (unsigned)atoi(e); const char* c = strchr(e, ','); if (c) w = (unsigned)atoi(c + 1); }
    return std::make_pair(l > 2 ? 0u : l, (w && (w < 2 || w > 5)) ? 0u : w);
  }();
  return pc_hip_srs_precompute_fold_ex(ctx, srs, form.first, form.second);
}
int pc_hip_srs_fold_table_info(const pc_srs* srs, unsigned* out_levels, unsigned* out_naf_width) {
  if (!srs) return PC_ERR_INVALID_ARG;
  if (out_levels) *out_levels = srs->fold_tbl ? srs->fold_levels : 0u;
  if (out_naf_width) *out_naf_width = srs->fold_tbl ? srs->fold_w : 0u;
  return PC_OK;
}

int pc_hip_srs_read(pc_ctx* ctx, const pc_srs* srs, size_t offset, size_t count, void* out_xy) { return key_base_read(ctx, srs, offset, count, out_xy); }

}  // extern "C"
