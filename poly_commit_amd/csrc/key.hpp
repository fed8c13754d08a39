// The key object (pc_srs) and everything that decides its lifetime: its context's registry, its MSM pipelines ("lanes"), its tables,
// and the derived keys an opening hangs on it (the working key it folds into, the fixed key of the late rounds).  Host code only, no
// kernels.  The units of the C ABI (abi_*.hip) go through the functions below: none of them touches parent, work_cache,
// fixed_cache, work_out or pc_ctx::keys, and none creates or deletes a pc_srs or an MsmLane.
// pc_srs (G1) and pc_g2_srs (G2) are two types over one base, pc_key_base: what only needs the base -- filling a key from the
// caller's points, reading it back, the registry of its context, the free under the context's lock -- is written once, over the
// base and the point size.
#pragma once
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include <stdlib.h>
#include <string.h>
#include "pc_internal.hpp"

// One independent MSM pipeline: own stream, own workspace.  Several lanes per SRS let the
// latency-bound tail of one MSM (segmented / bucket reduction, download, host Horner) overlap
// the bucket accumulation of the next.
struct MsmLane {
  pc::HipBackend be;
  pc::MsmRunner* runner = nullptr;
  struct pc_job* inflight = nullptr;
  ~MsmLane() { delete runner; be.destroy(); }
};

struct pc_ctx {
  std::map<std::pair<int, unsigned>, std::unique_ptr<pc::NttRunner>> ntt_plans;
  float ntt_phases[2] = {0, 0};
  float ligero_phases[4] = {0, 0, 0, 0};
  int device = 0;
  pc::HipBackend be;
  std::recursive_mutex mu;   // recursive: the fused entry points call the single-step ones
  std::string last_error;
  pc::MsmConfig msm_cfg;
  float phases[8] = {0};
  float marks[8] = {0};          // the same marks as offsets from `epoch` (pc_hip_last_msm_marks_ms)
  hipEvent_t epoch = nullptr;    // recorded by pc_hip_set_timing(on)
  uint32_t shape[4] = {0};
  // pc_hip_ligero_commit in row slabs: the slab buffers (grow-only up to LIGERO_KEEP, pc_hip_ctx_trim frees them) and the queue of the way out
  void* lig_arena = nullptr; size_t lig_bytes = 0; hipStream_t lig_out_q[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<struct pc_srs*> keys;   // every key object of this context that is alive (pc_hip_ctx_bytes_resident, pc_hip_ctx_trim)
  // pc_hip_ipa_open_rounds: the powers of z, the per-base factors of the fixed key and the two scalar vectors of its rounds (grow-only, pc_hip_ctx_trim frees them)
  void* ipa_buf[3] = {nullptr, nullptr, nullptr}; size_t ipa_bytes[3] = {0, 0, 0};
  std::vector<struct pc_g2_srs*> g2_keys;   // every G2 key object of this context that is alive (the functions at the end of this header own them)
  std::vector<struct pc_te_srs*> te_keys;   // every twisted Edwards key object of this context that is alive (the functions at the end of this header own them)
  std::vector<struct pc_lincode*> codes;   // every Brakedown code object of this context that is alive; abi_lincode.hip alone creates and releases them
  float brakedown_phases[4] = {0, 0, 0, 0};
  uint32_t skzg_launches[2] = {0, 0};      // kernel launches of the last streaming_kzg call: [folding tree, divisions + combination] (pc_hip_last_skzg_launches)
  uint32_t pst13_shape[2 + 32] = {0};      // the last pc_hip_pst13_open: [MSMs, 1 = the univariate route, pairs of MSM 0, 1, ..] (pc_hip_last_pst13_shape)
};

// What a key of either group is: n affine points resident on the device, registered in its context
struct pc_key_base {
  pc_ctx* ctx = nullptr;         // null: the context was shut down under the key (a tombstone: nothing left to release)
  pc_curve curve = PC_CURVE_BLS12_381;
  size_t n = 0;
  uint32_t* bases = nullptr;     // packed coordinates: x||y (G1), x.c0 || x.c1 || y.c0 || y.c1 (G2); all zero = infinity.  A twisted Edwards key: x || y || 2dxy
  int aw = 0;                    // words per affine point
};

// Independent pipelines per SRS (stream + workspace each), used round-robin; a pipeline that still
// holds a job is drained before it is reused.
static constexpr int PC_MSM_LANES = 3;
struct pc_srs : pc_key_base {
  uint32_t* table = nullptr;     // precomputed window table (pc_hip_srs_precompute), or null
  uint32_t* fold_tbl = nullptr;  // fold table (pc_hip_srs_precompute_fold[_ex]) of the key points [fold_half, fold_half + fold_pts), or null
  size_t fold_half = 0;          // points of the key the table leaves out = size of the key it folds to: n / 2 (one level) or n / 4 (two)
  size_t fold_pts = 0;           // points per table row: n / 2 or 3 n / 4
  uint32_t fold_levels = 0, fold_w = 2;   // folds the table serves in one step; width of the NAF digits it holds the odd multiples for
  // pc_hip_ec_fold_from: the half-size working key of an opening keeps its buffers and pipelines across openings -- freeing it
  // hands it back to the committer key it was folded from (a fresh key cost ~4 ms of pipeline workspace allocation per opening)
  pc_srs* parent = nullptr;      // the key this one was folded from (while that key is alive)
  pc_srs* work_cache = nullptr;  // a returned working key, ready for reuse
  pc_srs* fixed_cache = nullptr; // pc_hip_ipa_open_rounds: the key object of the late rounds' FIXED key (n0 points, its window table, its pipelines), refilled by every opening
  pc_srs* work_out = nullptr;    // the working key currently handed out
  pc::MsmConfig cfg;
  int in_subgroup = -1;          // pc_hip_srs_in_subgroup's cached answer (-1: not known); whoever rewrites the points resets it
  MsmLane* lanes[PC_MSM_LANES] = {nullptr, nullptr, nullptr};
  int next_lane = 0;
  // pc_hip_msm_many: window table of bases[base_offset .. base_offset + m) and the pipeline sized for B x m
  struct Many { size_t base_offset = 0, m = 0, B = 0; uint32_t* table = nullptr; MsmLane* lane = nullptr; } many;
  // pc_hip_msm_batch over the window table: G polynomials of m coefficients per pass, one bucket set each (two pipelines)
  struct BatchMany { size_t m = 0, G = 0; MsmLane* lanes[2] = {nullptr, nullptr}; uint32_t* stage[2] = {nullptr, nullptr}; } bm;      // stage: device copies of one pass's HOST polynomials
};
struct pc_job {
  pc_srs* srs = nullptr; int lane = 0;
  uint32_t* out_xy = nullptr; int* out_inf = nullptr;
  bool done = false; int status = 0;
};

inline int fq_bytes(pc_curve c) { return (int)pc_fq_bytes(c); }
// the affine encoding of the point at infinity: all words zero
inline bool affine_is_zero(const uint32_t* xy, int aw) { uint32_t acc = 0; for (int i = 0; i < aw; i++) acc |= xy[i]; return acc == 0; }
// windows of the key's table: the 255-bit scalar's, or those of its 130-bit GLV halves
inline uint32_t table_windows(const pc_srs* srs, uint32_t c, bool glv) {
  return pc::msm_num_windows(glv ? pc::GLV_HALF_BITS : pc::curve_ops(srs->curve).scalar_bits, c);
}

template <class Fn>
static int guarded(pc_ctx* ctx, Fn fn) {
  try {
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return PC_ERR_HIP; }
    return fn();
  } catch (const pc::HipError& e) {
    ctx->last_error = e.what();
    return e.code == hipErrorOutOfMemory ? PC_ERR_OOM : PC_ERR_HIP;
  } catch (const pc::MsmCapacityError& e) {
    ctx->last_error = e.what(); return PC_ERR_TOO_LARGE;
  } catch (const std::bad_alloc&) {
    ctx->last_error = "host allocation failed"; return PC_ERR_OOM;
  } catch (const std::exception& e) {
    ctx->last_error = e.what(); return PC_ERR_HIP;
  }
}

// ---- what the keys of both groups share (K: pc_srs or pc_g2_srs) -----------------------------

// A key object of n points of point_bytes each with its bases buffer, registered in `registry`.  Call inside guarded(): a failed
// device allocation throws, with the object already released by free_key.  Null: no host memory.
template <class K, class Free>
inline K* key_base_create(std::vector<K*>& registry, pc_ctx* ctx, pc_curve curve, size_t n, size_t point_bytes, Free free_key) {
  K* k = new (std::nothrow) K();
  if (!k) return nullptr;
  k->ctx = ctx; k->curve = curve; k->n = n; k->aw = (int)(point_bytes / 4);
  registry.push_back(k);
  try { k->bases = (uint32_t*)ctx->be.alloc((n ? n : 1) * point_bytes); }
  catch (...) { free_key(k); throw; }
  return k;
}
// out of the registry, bases buffer freed (the context is alive)
template <class K>
inline void key_base_release(std::vector<K*>& registry, K* k) {
  registry.erase(std::remove(registry.begin(), registry.end(), k), registry.end());
  if (k->bases) k->ctx->be.free(k->bases);
  k->bases = nullptr; k->n = 0;
}
// pc_hip_shutdown: every key still alive gives up what it holds on the device and stays behind as a tombstone
template <class K, class Release>
inline void key_registry_shutdown(std::vector<K*>& registry, Release release_device) {
  const std::vector<K*> alive = registry;
  for (K* k : alive) { release_device(k); k->ctx = nullptr; }
  registry.clear();
}
// pc_hip_[g2_]srs_free: under the context's lock, or -- the context is gone, and its mutex with it -- just the tombstone
template <class K, class Free>
inline void key_free_locked(K* k, Free free_key) {
  if (!k) return;
  if (k->ctx) { std::lock_guard<std::recursive_mutex> lk(k->ctx->mu); free_key(k); }
  else free_key(k);
}
// Fill the key from the caller's n points (inside guarded()): device memory or packed host memory as they are; a host array of
// Rust Affine{x, y, infinity} (stride > point bytes) is repacked, the flag byte behind the coordinates mapped to the all-zero encoding
inline void key_base_fill(pc_key_base* k, const void* points, size_t n, size_t stride_bytes, pc_mem where) {
  if (!n) return;
  pc::HipBackend& be = k->ctx->be;
  const size_t pb = (size_t)k->aw * 4;
  if (where == PC_MEM_DEVICE) be.copy_d2d(k->bases, points, n * pb);
  else if (stride_bytes == pb) be.copy_h2d(k->bases, points, n * pb);
  else {
    std::vector<uint8_t> packed(n * pb);
    const uint8_t* src = (const uint8_t*)points;
    for (size_t i = 0; i < n; i++) {
      const uint8_t* p = src + i * stride_bytes;
      if (p[pb]) memset(&packed[i * pb], 0, pb); else memcpy(&packed[i * pb], p, pb);
    }
    be.copy_h2d(k->bases, packed.data(), n * pb);
    be.sync();                                 // `packed` goes out of scope
  }
  be.sync();
}
// points [offset, offset + count) of the key to the host: a whole entry point (pc_hip_srs_read, pc_hip_g2_srs_read)
inline int key_base_read(pc_ctx* ctx, const pc_key_base* k, size_t offset, size_t count, void* out_host) {
  if (!ctx || !k || k->ctx != ctx || offset > k->n || count > k->n - offset || (count && !out_host)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (count) ctx->be.copy_d2h(out_host, k->bases + offset * (size_t)k->aw, count * (size_t)k->aw * 4);
    return (int)PC_OK;
  });
}

// ---- lanes and jobs --------------------------------------------------------------------------

// lane i of the key's own pipelines, created on first use
inline MsmLane* srs_lane(pc_srs* srs, int i) {
  if (srs->lanes[i]) return srs->lanes[i];
  MsmLane* L = new MsmLane();
  try {
    // CU-partitioned pipelines are opt-in (PC_HIP_SPLIT_CUS=1): on this part a masked stream lost far
    // more throughput than the share of CUs it gave up (accumulate 3.65 ms on 256 CUs, 6.8 ms on 240).
    static const bool split = []() { const char* e = getenv("PC_HIP_SPLIT_CUS"); return e && e[0] == '1'; }();
    // default on; PC_HIP_TAIL_PRIO=0 puts a pipeline back on one queue (measured 8.5-9.0 -> 7.7 ms/step at 2^20)
    static const bool tsplit = []() { const char* e = getenv("PC_HIP_TAIL_PRIO"); return !(e && e[0] == '0'); }();
    // (pipelines of a large SRS keep one plain queue: the split only pays up to ~2^20 pairs per call, and
    // priority-created streams measured 5 % slower at 2^22 even with the split unused)
    L->be.tail_split = tsplit && srs->n <= ((size_t)3 << 19);
    if (i == 0 || !split) L->be.init(); else L->be.init(i - 1, PC_MSM_LANES - 1);
    L->runner = pc::curve_ops(srs->curve).make_runner(L->be, srs->n, srs->cfg, 0);
  } catch (...) { delete L; throw; }
  srs->lanes[i] = L;
  return L;
}

// a pipeline of its own kind for the key's curve (pc_hip_msm_many, the passes of pc_hip_msm_batch): `sets` bucket sets over `capacity` pairs
inline MsmLane* new_lane(pc_curve curve, size_t capacity, const pc::MsmConfig& cfg, uint32_t sets) {
  MsmLane* L = new MsmLane();
  try { L->be.init(); L->runner = pc::curve_ops(curve).make_runner(L->be, capacity, cfg, sets); }
  catch (...) { delete L; throw; }
  return L;
}

// shape and phase brackets of the lane's last call (pc_hip_last_msm_shape, pc_hip_last_msm_phases_ms); Lane: MsmLane or BlockingLane
template <class Lane>
inline void lane_phases(pc_ctx* ctx, Lane* L) {
  for (int i = 0; i < 8; i++) ctx->phases[i] = 0;
  L->runner->shape(ctx->shape);
  if (L->be.timing) for (int i = 0; i + 1 < L->be.n_ev && i < 8; i++) (void)hipEventElapsedTime(&ctx->phases[i], L->be.ev[i], L->be.ev[i + 1]);
}
// Finish the job occupying a lane: wait for its stream, host tail, outputs, phase times.
inline void complete_job(pc_ctx* ctx, pc_job* job) {
  pc_srs* srs = job->srs;
  MsmLane* L = srs->lanes[job->lane];
  // Whatever happens below (finish() may throw on a HIP error), the lane must not keep a pointer to this
  // job: it may live on the caller's stack (pc_hip_msm, pc_hip_msm_batch) or be deleted by pc_hip_job_wait.
  L->inflight = nullptr; job->done = true; job->status = PC_ERR_HIP;
  L->runner->finish(job->out_xy);
  if (job->out_inf) *job->out_inf = affine_is_zero(job->out_xy, srs->aw);
  lane_phases(ctx, L);
  for (int i = 0; i < 8; i++) ctx->marks[i] = -1.0f;
  if (L->be.timing && ctx->epoch) for (int i = 0; i < L->be.n_ev && i < 8; i++) (void)hipEventElapsedTime(&ctx->marks[i], ctx->epoch, L->be.ev[i]);
  job->status = PC_OK;
}

// a job on this call's stack must not outlive it inside a pipeline (an exception between two enqueues would leave the lane with a
// dangling pointer): completed on scope exit if it still is in flight
struct StackJob {
  pc_ctx* ctx; pc_job job;
  explicit StackJob(pc_ctx* c) : ctx(c) {}
  ~StackJob() { if (job.srs && !job.done) { try { complete_job(ctx, &job); } catch (...) {} } }
};

// Claim lane li of the key for `job` (completing whatever that lane still holds); the caller queues the work and sets L->inflight.
inline MsmLane* claim_lane(pc_ctx* ctx, pc_srs* srs, int li, void* out_xy, int* out_is_infinity, pc_job* job) {
  MsmLane* L = srs_lane(srs, li);
  if (L->inflight) complete_job(ctx, L->inflight);
  L->be.timing = ctx->be.timing;
  job->srs = srs; job->lane = li; job->out_xy = (uint32_t*)out_xy; job->out_inf = out_is_infinity; job->done = false;
  return L;
}

// Queue one MSM on the next lane (completing whatever that lane still holds).
inline int enqueue_job(pc_ctx* ctx, pc_srs* srs, size_t base_offset, const void* scalars, pc_scalar_form form, pc_mem where,
                size_t n, void* out_xy, int* out_is_infinity, pc_job* job) {
  if (base_offset > srs->n) return PC_ERR_INVALID_ARG;
  size_t avail = srs->n - base_offset;     // msm_bigint semantics: min(bases.len(), scalars.len()) pairs
  if (n > avail) n = avail;
  if (n && !scalars) return PC_ERR_INVALID_ARG;
  int li = srs->next_lane; srs->next_lane = (srs->next_lane + 1) % PC_MSM_LANES;
  MsmLane* L = claim_lane(ctx, srs, li, out_xy, out_is_infinity, job);
  L->runner->enqueue(srs->bases, (uint32_t)base_offset, scalars, where, n, form == PC_SCALARS_MONTGOMERY);
  L->inflight = job;
  return PC_OK;
}

// Complete what every lane of the key still holds.  swallow_errors: every lane is tried, nothing is thrown (the free path).
inline void key_drain(pc_srs* srs, bool swallow_errors = false) {
  for (int i = 0; i < PC_MSM_LANES; i++) {
    if (!srs->lanes[i] || !srs->lanes[i]->inflight) continue;
    if (!swallow_errors) complete_job(srs->ctx, srs->lanes[i]->inflight);
    else { try { complete_job(srs->ctx, srs->lanes[i]->inflight); } catch (...) {} }
  }
}

inline void key_delete_lanes(pc_srs* srs) {
  for (int i = 0; i < PC_MSM_LANES; i++) { delete srs->lanes[i]; srs->lanes[i] = nullptr; }
}

// ---- tables ----------------------------------------------------------------------------------

inline void drop_many(pc_srs* srs) {
  delete srs->many.lane; srs->many.lane = nullptr;
  if (srs->many.table) srs->ctx->be.free(srs->many.table);
  srs->many.table = nullptr; srs->many.m = srs->many.B = srs->many.base_offset = 0;
}

inline void drop_batch_many(pc_srs* srs) {
  for (int i = 0; i < 2; i++) {
    if (srs->bm.stage[i] && srs->bm.lanes[i]) srs->bm.lanes[i]->be.free(srs->bm.stage[i]);
    srs->bm.stage[i] = nullptr;
    delete srs->bm.lanes[i]; srs->bm.lanes[i] = nullptr;
  }
  srs->bm.m = srs->bm.G = 0;
}

// Forget the window table of an SRS (and the pipelines sized for it).  No job may be in flight.
inline void drop_table(pc_srs* srs) {
  drop_batch_many(srs);
  if (!srs->table) return;
  key_delete_lanes(srs);
  srs->ctx->be.free(srs->table); srs->table = nullptr;
  srs->cfg.tbl = nullptr; srs->cfg.tbl_c = 0; srs->cfg.tbl_stride = 0; srs->cfg.tbl_min_n = 0; srs->cfg.tbl_glv = false;
}

inline void drop_fold_table(pc_srs* srs) {
  if (srs->fold_tbl) srs->ctx->be.free(srs->fold_tbl);
  srs->fold_tbl = nullptr; srs->fold_half = srs->fold_pts = 0; srs->fold_levels = 0; srs->fold_w = 2;
}

// ---- lifetime (the context's lock is held by the caller) ------------------------------------

// everything a key holds on the device and in its context's books; the host object is left empty (a key whose context was shut down
// under it has ctx == nullptr and nothing left to release)
inline void key_release_device(pc_srs* srs) {
  if (!srs->ctx) return;
  (void)hipSetDevice(srs->ctx->device);
  for (int i = 0; i < PC_MSM_LANES; i++)
    if (srs->lanes[i] && srs->lanes[i]->inflight) {   // abandon: let the stream drain, mark the job failed
      (void)hipStreamSynchronize(srs->lanes[i]->be.stream);
      if (srs->lanes[i]->be.tail_stream) (void)hipStreamSynchronize(srs->lanes[i]->be.tail_stream);
      srs->lanes[i]->inflight->done = true; srs->lanes[i]->inflight->status = PC_ERR_INVALID_ARG;
    }
  key_delete_lanes(srs);
  drop_fold_table(srs);
  drop_batch_many(srs);
  if (srs->table) srs->ctx->be.free(srs->table);
  drop_many(srs);
  srs->table = nullptr;
  key_base_release(srs->ctx->keys, srs);      // last: it zeroes n and bases
}

// the derived keys that `owners` cache (every work_cache, then every fixed_cache), detached from them
inline std::vector<pc_srs*> detach_cached(const std::vector<pc_srs*>& owners) {
  std::vector<pc_srs*> cached;
  for (pc_srs* s : owners) if (s->work_cache) { cached.push_back(s->work_cache); s->work_cache = nullptr; }
  for (pc_srs* s : owners) if (s->fixed_cache) { cached.push_back(s->fixed_cache); s->fixed_cache = nullptr; }
  return cached;
}

// Free a key: a working key goes back to its committer key's cache if that is empty; anything else is released with every derived key
// it still caches.
inline void key_free(pc_srs* srs) {
  if (srs->parent) {                                   // a working key goes back to its committer key (see pc_srs)
    pc_srs* par = srs->parent;
    key_drain(srs, true);                              // nothing of it may still be queued
    if (par->work_out == srs) par->work_out = nullptr;
    if (!par->work_cache) { par->work_cache = srs; return; }
    srs->parent = nullptr;                             // the cache is taken: a real free
  }
  for (pc_srs* d : detach_cached({srs})) { d->parent = nullptr; key_free(d); }
  if (srs->work_out) { srs->work_out->parent = nullptr; srs->work_out = nullptr; }      // still held by the caller: it frees it
  key_release_device(srs);
  delete srs;
}

// Free a derived key for real, whatever its parent's cache holds.
inline void key_free_derived(pc_srs* srs) {
  srs->parent = nullptr;
  key_free(srs);
}

// A key object of n points of `curve` with its bases buffer, registered in its context, cfg = the context's.  Call inside guarded():
// a failed device allocation throws, with the object already released.  Null: no host memory.
inline pc_srs* key_create(pc_ctx* ctx, pc_curve curve, size_t n) {
  pc_srs* srs = key_base_create(ctx->keys, ctx, curve, n, 2 * (size_t)fq_bytes(curve), key_free);
  if (srs) srs->cfg = ctx->msm_cfg;
  return srs;
}

// pc_hip_ec_fold_from / pc_hip_ec_fold2_from: take the working key of `count` points that an opening folds the committer key `par`
// into -- the one the last opening handed back (it keeps its buffers and pipelines), or a new one; a cached one of another size stays
// where it is --, let `fold(dst)` write its points, and hand it out: if par has none out, freeing it returns it to par's cache.
// A whole entry point: takes the context's lock itself.
template <class Fold>
inline int key_fold_to_working(pc_ctx* ctx, pc_srs* par, size_t count, pc_srs** out, Fold fold) {
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  pc_srs* dst = nullptr;
  int rc = guarded(ctx, [&]() {
    const bool fresh = !(par->work_cache && par->work_cache->n == count);
    if (fresh) { dst = key_create(ctx, par->curve, count); if (!dst) return (int)PC_ERR_OOM; }
    else { dst = par->work_cache; par->work_cache = nullptr; drop_table(dst); drop_many(dst); }
    fold(dst);
    dst->in_subgroup = par->in_subgroup == 1 ? 1 : -1;      // sums of multiples of subgroup points
    if (fresh) for (int i = 0; i < PC_MSM_LANES; i++) srs_lane(dst, i);      // all pipelines now: the next rounds' MSMs find them ready
    return (int)PC_OK;
  });
  if (rc != PC_OK) { if (dst) key_free_derived(dst); return rc; }
  if (!par->work_out) { dst->parent = par; par->work_out = dst; } else dst->parent = nullptr;
  *out = dst;
  return PC_OK;
}
// Make such a working key ahead of the first opening and leave it in par's cache (pc_hip_srs_precompute_fold_ex); failure is silent.
inline void key_premake_working(pc_ctx* ctx, pc_srs* par, size_t count) {
  if (par->work_cache || par->parent || count < 2) return;
  pc_srs* wk = nullptr;
  try {
    wk = key_create(ctx, par->curve, count);
    if (!wk) return;
    ctx->be.memset(wk->bases, 0, count * (size_t)wk->aw * 4);      // points at infinity until an opening folds into it
    for (int i = 0; i < PC_MSM_LANES; i++) srs_lane(wk, i);
    ctx->be.sync();
    wk->parent = par; par->work_cache = wk;
  } catch (...) { if (wk) key_free_derived(wk); (void)hipGetLastError(); }      // no memory for it now: the opening will try again
}

// The fixed key of an opening: the key object whose first n0 points are src's first n0 and whose window table is current, creating or
// refilling root->fixed_cache; null on any failure (nothing half-made is kept).
// The fixed key serves 2 log2(n0) + 1 MSMs of n0 pairs: with a window table (one shared bucket set, fewer digits) each costs
// ~0.15 ms less.  The table lives in a key object that belongs to the committer key and is REFILLED by every opening (points
// copied on the device, table rebuilt in place: no allocation, the pipelines and their captured launch graphs stay): building a
// new key with its table per opening cost 7-8 ms (EXPERIMENTS 00), refilling one costs what its kernels take.
inline pc_srs* key_fixed(pc_ctx* ctx, pc_srs* root, const pc_srs* src, size_t n0) {
  const int rc = guarded(ctx, [&]() {
    pc_srs* fk = root->fixed_cache;
    if (fk && fk->n != n0) { root->fixed_cache = nullptr; key_free(fk); fk = nullptr; }
    if (!fk) {
      fk = key_create(ctx, root->curve, n0);
      if (!fk) throw std::bad_alloc();
      root->fixed_cache = fk;
    }
    ctx->be.copy_d2d(fk->bases, src->bases, n0 * (size_t)root->aw * 4);
    fk->in_subgroup = src->in_subgroup == 1 ? 1 : -1;
    static const unsigned fixed_c = []() { const char* e = getenv("PC_HIP_IPA_FIXED_C"); int v = e ? atoi(e) : 0; return (unsigned)(v >= 4 && v <= 22 ? v : 0); }();      // measurements: the table's window width
    if (!fk->table) return pc_hip_srs_precompute_ex(ctx, fk, fixed_c, 1, 0);                    // first opening: table, pipelines (full form: the key is small)
    key_drain(fk);
    pc::curve_ops(root->curve).window_table(ctx->be, fk->bases, (uint32_t)n0, fk->cfg.tbl_c, table_windows(fk, fk->cfg.tbl_c, false), fk->table, fk->cfg.tbl_pt_stride);
    return (int)PC_OK;
  });
  if (rc == PC_OK) return root->fixed_cache;
  (void)hipGetLastError();                                                                      // a half-made object is not kept: the next opening starts over
  if (pc_srs* fk = root->fixed_cache) { root->fixed_cache = nullptr; (void)guarded(ctx, [&]() { key_free(fk); return (int)PC_OK; }); }
  return nullptr;
}

// pc_hip_shutdown: release every key of the context
inline void keys_shutdown(pc_ctx* ctx) {
  // Keys that outlive their context (Drop order of an Arc<ResidentKey> against the context, a Python object collected late): their
  // device memory and pipelines go now, the host object stays behind as a tombstone (ctx = nullptr) that a later pc_hip_srs_free
  // only deletes -- it must never lock a mutex inside the context deleted below.  Cached working keys are held by nobody: deleted.
  const std::vector<pc_srs*> cached = detach_cached(ctx->keys);
  for (pc_srs* s : ctx->keys) { s->parent = nullptr; s->work_out = nullptr; }
  key_registry_shutdown(ctx->keys, key_release_device);
  for (pc_srs* s : cached) delete s;
}

// pc_hip_ctx_trim's share of the keys
inline void keys_trim(pc_ctx* ctx) {
  // working keys that an opening handed back (pc_hip_ec_fold_from keeps one per committer key, with its three pipelines)
  for (pc_srs* w : detach_cached(ctx->keys)) key_free_derived(w);
  // idle pipelines give their sort / scan scratch back (the plan's own workspace stays: it is what makes the next call cheap)
  for (pc_srs* s : ctx->keys)
    for (int i = 0; i < PC_MSM_LANES; i++)
      if (s->lanes[i] && !s->lanes[i]->inflight) { s->lanes[i]->be.sync(); s->lanes[i]->be.trim(); if (s->lanes[i]->runner) s->lanes[i]->runner->trim(); }
  // the staging copies of HOST polynomials in the batch pipelines (pc_hip_msm_batch: 2 x 8 polynomials)
  for (pc_srs* s : ctx->keys)
    for (int i = 0; i < 2; i++)
      if (s->bm.stage[i] && s->bm.lanes[i]) { s->bm.lanes[i]->be.sync(); s->bm.lanes[i]->be.free(s->bm.stage[i]); s->bm.stage[i] = nullptr; }
}

// ---- residency -------------------------------------------------------------------------------

inline size_t lane_bytes(const MsmLane* L) { return L ? L->be.bytes_live : 0; }
// {bases, window tables, fold table, lanes} bytes of one key
inline void key_bytes(const pc_srs* s, size_t out[4]) {
  const size_t pb = (size_t)s->aw * 4;
  out[0] = (s->n ? s->n : 1) * pb;
  out[1] = 0;
  if (s->table) out[1] = (size_t)table_windows(s, s->cfg.tbl_c, s->cfg.tbl_glv) * s->n * s->cfg.tbl_pt_stride * 4;
  if (s->many.table) { const uint32_t bits = pc::curve_ops(s->curve).scalar_bits; out[1] += (size_t)pc::msm_num_windows(bits, pc::msm_choose_table_c(s->many.m, bits, 0)) * s->many.m * pb; }
  out[2] = s->fold_tbl ? ((size_t)pc::curve_ops(s->curve).fold_rows << (s->fold_w - 2)) * s->fold_pts * pb : 0;
  out[3] = 0;
  for (int i = 0; i < PC_MSM_LANES; i++) out[3] += lane_bytes(s->lanes[i]);
  out[3] += lane_bytes(s->many.lane) + lane_bytes(s->bm.lanes[0]) + lane_bytes(s->bm.lanes[1]);
}

// sums of the first three over the context's keys; returns the number of keys
inline size_t keys_bytes(const pc_ctx* ctx, size_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  for (const pc_srs* s : ctx->keys) {
    size_t b[4]; key_bytes(s, b);
    out[0] += b[0]; out[1] += b[1]; out[2] += b[2];
  }
  return ctx->keys.size();
}

// ---- blocking lanes --------------------------------------------------------------------------
// One blocking MSM pipeline of a G2 or twisted Edwards key: own queue, own workspace, no job in flight between calls.  The unit of the
// group makes it (blocking_lane.hpp); what needs no group is here.
struct BlockingLane {
  pc::HipBackend be;
  pc::BlockingRunner* runner = nullptr;
  ~BlockingLane() { delete runner; be.destroy(); }
};
inline size_t lane_bytes(const BlockingLane* L) { return L ? L->be.bytes_live : 0; }
// pc_hip_ctx_trim's share: an idle pipeline gives its sort / scan scratch back
inline void lane_trim(BlockingLane* L) { if (L) { L->be.sync(); L->be.trim(); } }

// The frame of an entry point that hands out one new key or nothing: *out = null; under the context's lock and inside guarded(),
// create() makes the key object (null: no host memory) and fill(k) writes its points (returns a status, may throw); on any failure the
// key is freed again.  K: pc_g2_srs or pc_te_srs.
template <class K, class Create, class Free, class Fill>
inline int key_make(pc_ctx* ctx, K** out, Create create, Free free_key, Fill fill) {
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  K* k = nullptr;
  int rc = guarded(ctx, [&]() {
    k = create();
    return k ? (int)fill(k) : (int)PC_ERR_OOM;
  });
  if (rc != PC_OK) { if (k) free_key(k); return rc; }
  *out = k;
  return PC_OK;
}

// ---- G2 keys ---------------------------------------------------------------------------------
// A key of G2 points (pc_hip_g2_srs_upload; MultilinearPC's powers_of_h and their pair sums): a type of its own, so that no G1 entry
// point can be handed one.  Same rules as pc_srs: registered in its context, released with it (the host object then stays behind as a
// tombstone with ctx == nullptr that pc_hip_g2_srs_free only deletes); one pipeline, created on first use by abi_g2.hip.
struct pc_g2_srs : pc_key_base {
  BlockingLane* lane = nullptr;
};
inline int g2_point_bytes(pc_curve c) { return 4 * fq_bytes(c); }

inline void g2_key_release_device(pc_g2_srs* k) {
  if (!k->ctx) return;
  (void)hipSetDevice(k->ctx->device);
  delete k->lane; k->lane = nullptr;
  key_base_release(k->ctx->g2_keys, k);
}
inline void g2_key_free(pc_g2_srs* k) { g2_key_release_device(k); delete k; }
// call inside guarded(): a failed device allocation throws, with the object already released.  Null: no host memory.
inline pc_g2_srs* g2_key_create(pc_ctx* ctx, pc_curve curve, size_t n) {
  return key_base_create(ctx->g2_keys, ctx, curve, n, (size_t)g2_point_bytes(curve), g2_key_free);
}
// {bases, 0, 0, pipeline} bytes of one G2 key (the layout of key_bytes: G2 has no tables)
inline void g2_key_bytes(const pc_g2_srs* k, size_t out[4]) {
  out[0] = (k->n ? k->n : 1) * (size_t)k->aw * 4; out[1] = out[2] = 0;
  out[3] = lane_bytes(k->lane);
}
// pc_hip_shutdown's share
inline void g2_keys_shutdown(pc_ctx* ctx) { key_registry_shutdown(ctx->g2_keys, g2_key_release_device); }
inline void g2_keys_trim(pc_ctx* ctx) { for (pc_g2_srs* k : ctx->g2_keys) lane_trim(k->lane); }

// ---- twisted Edwards keys --------------------------------------------------------------------
// A key of ed_on_bls12_381 points (pc_hip_te_srs_upload): a type of its own, as pc_g2_srs is, so that no short Weierstrass entry point can
// be handed one -- its points have another law and no infinity.  Resident form: x || y || td with td = 2 d x y made at upload (te.hpp),
// 3 Fq = 96 bytes a point, where the caller's is 64; `aw` counts the resident words, `curve` is unused.  Same rules as pc_g2_srs:
// registered in its context, released with it (a tombstone stays behind), one pipeline, created on first use by abi_te.hip.
struct pc_te_srs : pc_key_base {
  pc_te_curve te_curve = PC_TE_ED_ON_BLS12_381;
  BlockingLane* lane = nullptr;
  uint32_t* fold_tbl = nullptr;  // fold table (pc_hip_te_srs_precompute_fold): fold_rows rows of the n / 2 upper points and their doublings, or null
  uint32_t fold_rows = 0;
  int in_subgroup = -1;          // pc_hip_te_srs_in_subgroup's cached answer (-1: not asked yet)
  // many-MSM pass (pc_hip_te_msm_many), cached per shape as pc_srs::Many is: the window table of bases[base_offset .. base_offset + m)
  // (Wd rows of m resident records, from the context's allocator) and a pipeline of its own with B bucket sets
  struct Many { size_t base_offset = 0, m = 0, B = 0; uint32_t* table = nullptr; size_t table_bytes = 0; BlockingLane* lane = nullptr; } many;
};
// the table and pipeline of the many-MSM pass go back: another shape is asked for, the key's points change (pc_hip_te_ec_fold), the key is released
inline void te_drop_many(pc_te_srs* k) {
  delete k->many.lane;
  if (k->many.table) k->ctx->be.free(k->many.table);
  k->many = pc_te_srs::Many();
}
inline void te_drop_fold_table(pc_te_srs* k) {
  if (k->fold_tbl) k->ctx->be.free(k->fold_tbl);
  k->fold_tbl = nullptr; k->fold_rows = 0;
}
inline size_t te_fold_table_bytes(const pc_te_srs* k) { return k->fold_tbl ? (size_t)k->fold_rows * (k->n / 2) * (size_t)k->aw * 4 : 0; }
inline void te_key_release_device(pc_te_srs* k) {
  if (!k->ctx) return;
  (void)hipSetDevice(k->ctx->device);
  delete k->lane; k->lane = nullptr;
  te_drop_fold_table(k);
  te_drop_many(k);
  key_base_release(k->ctx->te_keys, k);
}
inline void te_key_free(pc_te_srs* k) { te_key_release_device(k); delete k; }
// call inside guarded(): a failed device allocation throws, with the object already released.  Null: no host memory.
inline pc_te_srs* te_key_create(pc_ctx* ctx, pc_te_curve curve, size_t n, size_t resident_point_bytes) {
  pc_te_srs* k = key_base_create(ctx->te_keys, ctx, PC_CURVE_BLS12_381, n, resident_point_bytes, te_key_free);
  if (k) k->te_curve = curve;
  return k;
}
// {bases, window table of the many-MSM pass, fold table, pipelines} bytes of one key (the layout of key_bytes)
inline void te_key_bytes(const pc_te_srs* k, size_t out[4]) {
  out[0] = (k->n ? k->n : 1) * (size_t)k->aw * 4; out[1] = k->many.table_bytes; out[2] = te_fold_table_bytes(k);
  out[3] = lane_bytes(k->lane) + lane_bytes(k->many.lane);
}
inline void te_keys_shutdown(pc_ctx* ctx) { key_registry_shutdown(ctx->te_keys, te_key_release_device); }
inline void te_keys_trim(pc_ctx* ctx) { for (pc_te_srs* k : ctx->te_keys) { lane_trim(k->lane); lane_trim(k->many.lane); } }
