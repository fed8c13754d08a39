// C ABI of the gfx950 backend (include/pc_hip.h): the Brakedown linear code -- the resident code object (its whole lifetime is in this
// unit: created, registered with its context, released here and nowhere else), encode, commit.
#include <string.h>
#include "abi.hpp"

// The uploaded matrices of one code (BrakedownPCParams' a_mats / b_mats, brakedown.rs:52-55) and the points of its base code, in ONE
// device allocation; the host object is what the caller's handle points to.  A code whose context was shut down under it has
// ctx == nullptr and nothing left to release.  The caller's contract is the one of key objects: pc_hip_brakedown_code_free reads `ctx`
// before it can take that context's lock, so it must not race pc_hip_shutdown of the same context on another thread.
struct pc_lincode {
  pc_ctx* ctx = nullptr;
  pc_curve field = PC_CURVE_BLS12_381;
  pc::BrakedownDev dev;
  void* image = nullptr; size_t image_bytes = 0;
};

// the context's lock is held by the caller
static void lincode_release_device(pc_lincode* c) {
  if (!c->ctx) return;
  (void)hipSetDevice(c->ctx->device);
  (void)hipStreamSynchronize(c->ctx->be.stream);      // an encode of this code may still be queued
  { auto& cs = c->ctx->codes; cs.erase(std::remove(cs.begin(), cs.end(), c), cs.end()); }
  c->ctx->be.free(c->image); c->image = nullptr; c->image_bytes = 0;
}

void lincodes_shutdown(pc_ctx* ctx) {
  std::vector<pc_lincode*> alive = ctx->codes;
  for (pc_lincode* c : alive) { lincode_release_device(c); c->ctx = nullptr; }
  ctx->codes.clear();
}

static bool known_hash(pc_hash h) { return (int)h == PC_HASH_SHA256 || (int)h == PC_HASH_BLAKE2S; }

extern "C" {

int pc_hip_brakedown_code_create(pc_ctx* ctx, pc_curve field_of, size_t msg_len, size_t codeword_len, size_t n_levels, const size_t* dims,
                                 const size_t* ind_ptr, const uint32_t* col_ind, const void* val, size_t nnz, pc_lincode** out) {
  if (out) *out = nullptr;
  if (!ctx || !out || !pc_known_curve(field_of) || (nnz && !val)) return PC_ERR_INVALID_ARG;
  // everything about the arrays is decided on the host, before the device sees any of it
  pc::BrakedownLayout L;
  if (pc::brakedown_validate(msg_len, codeword_len, n_levels, dims, ind_ptr, col_ind, nnz, &L) != 0) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  pc_lincode* c = new (std::nothrow) pc_lincode();
  if (!c) return PC_ERR_OOM;
  int rc = guarded(ctx, [&]() {
    const pc::BrakedownImage im = pc::brakedown_image(L);
    std::vector<uint8_t> host(im.bytes ? im.bytes : 4, 0);
    std::vector<uint32_t> pts((L.rsoe - L.rss) * 8 + 8);
    pc::field_ops(field_of).brakedown_points(pts.data(), L.rsoe - L.rss);
    c->field = field_of;
    c->image = ctx->be.alloc(im.bytes); c->image_bytes = im.bytes;
    c->ctx = ctx; ctx->codes.push_back(c);
    pc::brakedown_fill(L, ind_ptr, col_ind, val, pts.data(), host.data(), (const uint8_t*)c->image, &c->dev);
    if (im.bytes) { ctx->be.copy_h2d(c->image, host.data(), im.bytes); ctx->be.sync(); }      // the library keeps no pointer into the caller's arrays
    return (int)PC_OK;
  });
  if (rc != PC_OK) { (void)guarded(ctx, [&]() { lincode_release_device(c); return (int)PC_OK; }); delete c; return rc; }
  *out = c;
  return PC_OK;
}

void pc_hip_brakedown_code_free(pc_lincode* code) {
  if (!code) return;
  if (code->ctx) { std::lock_guard<std::recursive_mutex> lk(code->ctx->mu); lincode_release_device(code); }
  delete code;
}

size_t pc_hip_brakedown_codeword_len(const pc_lincode* code) { return code ? code->dev.m_ext : 0; }

int pc_hip_brakedown_encode(pc_ctx* ctx, const pc_lincode* code, const void* msgs, pc_mem where_in, size_t rows, void* out, pc_mem where_out) {
  if (!ctx || !code || code->ctx != ctx || (rows && (!msgs || !out))) return PC_ERR_INVALID_ARG;
  const pc::BrakedownDev& D = code->dev;
  if (rows >= (1ull << 31) || rows * (uint64_t)D.work_len() >= (1ull << 32)) return PC_ERR_TOO_LARGE;      // one lane per element of the working buffer
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    for (float& p : ctx->brakedown_phases) p = 0;
    if (!rows) return (int)PC_OK;
    Staged sin(ctx->be, msgs, where_in, rows * (size_t)D.msg_len * 32, true, 0);
    Staged sout(ctx->be, out, where_out, rows * (size_t)D.m_ext * 32, false, 1);
    uint32_t* T = (uint32_t*)ctx->be.workspace(rows * (size_t)D.work_len() * 32);
    ctx->be.n_ev = 0; ctx->be.mark();
    pc::field_ops(code->field).brakedown_encode(ctx->be, D, (const uint32_t*)sin.dev, (uint32_t)rows, T, (uint32_t*)sout.dev);
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, rows * (size_t)D.m_ext * 32); else ctx->be.sync();
    if (ctx->be.timing && ctx->be.n_ev >= 3) {
      (void)hipEventElapsedTime(&ctx->brakedown_phases[0], ctx->be.ev[0], ctx->be.ev[1]);
      (void)hipEventElapsedTime(&ctx->brakedown_phases[1], ctx->be.ev[1], ctx->be.ev[2]);
    }
    return (int)PC_OK;
  });
}

int pc_hip_brakedown_commit(pc_ctx* ctx, const pc_lincode* code, const void* mat, pc_mem where_in, size_t rows, pc_hash col_hash, pc_hash tree_hash,
                            int len_prefix, void* ext_out, pc_mem where_ext, void* leaves_out_host, void* nodes_out_host) {
  if (!ctx || !code || code->ctx != ctx || !rows || !mat || !nodes_out_host || !known_hash(col_hash) || !known_hash(tree_hash)) return PC_ERR_INVALID_ARG;
  if (rows >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  const size_t N = code->dev.m_ext;
  unsigned h = 1; while (((size_t)1 << h) < N) h++;      // the tree pads the leaves to 2^h >= 2 (pc_hip_merkle_tree)
  void* ext = nullptr; void* leaves = nullptr; void* nodes = nullptr;
  const bool own_ext = !(ext_out && where_ext == PC_MEM_DEVICE);
  int rc = guarded(ctx, [&]() {
    ext = own_ext ? ctx->be.alloc(rows * N * 32) : ext_out;
    leaves = ctx->be.alloc(N * 32);
    nodes = ctx->be.alloc(((size_t)1 << h) * 32);
    return (int)PC_OK;
  });
  float ph[4] = {0, 0, 0, 0};
  if (rc == PC_OK) rc = pc_hip_brakedown_encode(ctx, code, mat, where_in, rows, ext, PC_MEM_DEVICE);
  if (rc == PC_OK) { ph[0] = ctx->brakedown_phases[0]; ph[1] = ctx->brakedown_phases[1]; }
  if (rc == PC_OK) rc = pc_hip_column_hash(ctx, code->field, ext, PC_MEM_DEVICE, rows, N, col_hash, leaves, PC_MEM_DEVICE);
  if (rc == PC_OK) ph[2] = ctx->ntt_phases[0];
  if (rc == PC_OK) rc = pc_hip_merkle_tree(ctx, tree_hash, leaves, PC_MEM_DEVICE, N, len_prefix, nodes, PC_MEM_DEVICE);
  if (rc == PC_OK) ph[3] = ctx->ntt_phases[0];
  if (rc == PC_OK) rc = guarded(ctx, [&]() {
    ctx->be.copy_d2h(nodes_out_host, nodes, (((size_t)1 << h) - 1) * 32);
    if (leaves_out_host) ctx->be.copy_d2h(leaves_out_host, leaves, N * 32);
    if (ext_out && where_ext == PC_MEM_HOST) ctx->be.copy_d2h(ext_out, ext, rows * N * 32);
    return (int)PC_OK;
  });
  (void)guarded(ctx, [&]() {
    if (own_ext && ext) ctx->be.free(ext);
    if (leaves) ctx->be.free(leaves);
    if (nodes) ctx->be.free(nodes);
    return (int)PC_OK;
  });
  memcpy(ctx->brakedown_phases, ph, sizeof ph);
  return rc;
}

int pc_hip_last_brakedown_phases_ms(const pc_ctx* ctx, float out[4]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  memcpy(out, ctx->brakedown_phases, sizeof ctx->brakedown_phases);
  return PC_OK;
}

}  // extern "C"
