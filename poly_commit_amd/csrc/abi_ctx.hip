// C ABI of the gfx950 backend (include/pc_hip.h): context lifetime, errors, device memory, residency and trim, timing.
#include "abi.hpp"

extern "C" {

int pc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pc_hip_init(int device_id, pc_ctx** out) {
  if (!out) return PC_ERR_INVALID_ARG;
  *out = nullptr;
  int n = pc_hip_device_count();
  if (n <= 0) return PC_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return PC_ERR_INVALID_ARG;
  pc_ctx* ctx = new (std::nothrow) pc_ctx();
  if (!ctx) return PC_ERR_OOM;
  ctx->device = device_id;
  int rc = guarded(ctx, [&]() { ctx->be.init(); return (int)PC_OK; });
  if (rc != PC_OK) { delete ctx; return rc; }
  *out = ctx;
  return PC_OK;
}

void pc_hip_shutdown(pc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  { std::lock_guard<std::recursive_mutex> lk(ctx->mu); keys_shutdown(ctx); g2_keys_shutdown(ctx); te_keys_shutdown(ctx); lincodes_shutdown(ctx); }
  ctx->ntt_plans.clear();
  if (ctx->epoch) (void)hipEventDestroy(ctx->epoch);
  for (hipStream_t q : ctx->lig_out_q) if (q) (void)hipStreamDestroy(q);
  ctx->be.free(ctx->lig_arena);
  for (int i = 0; i < 3; i++) ctx->be.free(ctx->ipa_buf[i]);
  ctx->be.destroy();
  delete ctx;
}

const char* pc_hip_strerror(int status) {
  switch (status) {
    case PC_OK: return "ok";
    case PC_ERR_INVALID_ARG: return "invalid argument";
    case PC_ERR_OOM: return "out of memory";
    case PC_ERR_HIP: return "HIP runtime error";
    case PC_ERR_NO_DEVICE: return "no HIP device";
    case PC_ERR_TOO_LARGE: return "problem too large for this build";
    case PC_ERR_UNSUPPORTED: return "unsupported";
    case PC_ERR_INTERNAL: return "internal error";
    default: return "unknown status";
  }
}
const char* pc_hip_last_error(const pc_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int pc_hip_set_msm_tuning(pc_ctx* ctx, unsigned window_bits, unsigned chunk) {
  if (!ctx || window_bits == 1 || window_bits > 24) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  ctx->msm_cfg.c = window_bits; ctx->msm_cfg.T = chunk;
  return PC_OK;
}

int pc_hip_malloc(pc_ctx* ctx, size_t bytes, void** out_dev) {
  if (!ctx || !out_dev) return PC_ERR_INVALID_ARG;
  *out_dev = nullptr;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() { *out_dev = ctx->be.alloc(bytes); return (int)PC_OK; });
}
int pc_hip_free(pc_ctx* ctx, void* dev) {
  if (!ctx) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() { ctx->be.free(dev); return (int)PC_OK; });
}
int pc_hip_memcpy_h2d(pc_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
  if (!ctx || (bytes && (!dst_dev || !src_host))) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() { if (bytes) { ctx->be.copy_h2d(dst_dev, src_host, bytes); ctx->be.sync(); } return (int)PC_OK; });
}
int pc_hip_memcpy_d2h(pc_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
  if (!ctx || (bytes && (!dst_host || !src_dev))) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() { if (bytes) ctx->be.copy_d2h(dst_host, src_dev, bytes); return (int)PC_OK; });
}

int pc_hip_ctx_bytes_resident(pc_ctx* ctx, size_t out[6]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  for (int i = 0; i < 6; i++) out[i] = 0;
  out[0] = pc::dev_bytes_held(ctx->device);
  out[5] = keys_bytes(ctx, out + 1) + ctx->g2_keys.size() + ctx->te_keys.size();      // (G2 and twisted Edwards keys: counted here and, through the ledger, in out[0])
  for (const pc_te_srs* k : ctx->te_keys) { out[2] += k->many.table_bytes; out[3] += te_fold_table_bytes(k); }      // their window tables (pc_hip_te_msm_many) and fold tables (pc_hip_te_srs_precompute_fold)
  out[4] = ctx->be.scratch_bytes();
  return PC_OK;
}
int pc_hip_ctx_trim(pc_ctx* ctx) {
  if (!ctx) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    ctx->be.sync();
    ctx->be.trim();
    ctx->ntt_plans.clear();
    ctx->be.free(ctx->lig_arena); ctx->lig_arena = nullptr; ctx->lig_bytes = 0;      // pc_hip_ligero_commit's slab buffers
    for (int i = 0; i < 3; i++) { ctx->be.free(ctx->ipa_buf[i]); ctx->ipa_buf[i] = nullptr; ctx->ipa_bytes[i] = 0; }      // pc_hip_ipa_open_rounds' vectors
    keys_trim(ctx);
    g2_keys_trim(ctx);
    te_keys_trim(ctx);
    return (int)PC_OK;
  });
}

int pc_hip_set_timing(pc_ctx* ctx, int on) {
  if (!ctx) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    ctx->be.timing = on != 0;
    if (on) {     // the reference point of pc_hip_last_msm_marks_ms
      if (!ctx->epoch) PC_HIP_CHECK(hipEventCreate(&ctx->epoch));
      PC_HIP_CHECK(hipEventRecord(ctx->epoch, ctx->be.stream));
      PC_HIP_CHECK(hipEventSynchronize(ctx->epoch));
    }
    return (int)PC_OK;
  });
}

int pc_hip_last_msm_marks_ms(const pc_ctx* ctx, float out[8]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  for (int i = 0; i < 8; i++) out[i] = ctx->marks[i];
  return PC_OK;
}

int pc_hip_last_msm_phases_ms(const pc_ctx* ctx, float out[8]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  for (int i = 0; i < 8; i++) out[i] = ctx->phases[i];
  return PC_OK;
}

int pc_hip_last_msm_shape(const pc_ctx* ctx, uint32_t out[4]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  for (int i = 0; i < 4; i++) out[i] = ctx->shape[i];
  return PC_OK;
}

}  // extern "C"
