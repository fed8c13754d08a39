// C ABI of the gfx950 backend (include/pc_hip.h): MSM -- single, asynchronous, batch, many, the parts of host scalars, KZG open.
#include <string.h>
#include "abi.hpp"

// Scalars that arrive in HOST memory are copied inside the call (the trait hands over &[F]: 512 MB at degree 2^24, ~9 ms of PCIe).
// Every step of one MSM needs all of its scalars, so nothing of that MSM can hide the copy -- but the MSM is a sum: from
// host_split_min() pairs on (2^21: measured gains 8 % / 17 % / 17 % / 14 % of a commit at 2^21 / 2^22 / 2^23 / 2^24, a loss at 2^20),
// the call runs in parts over index ranges (host_part_cuts below).
static size_t host_split_min() {
  static const size_t v = []() { const char* e = getenv("PC_HIP_HOST_SPLIT_LOG2"); int lg = e ? atoi(e) : 21; return lg <= 0 ? (size_t)-1 : (size_t)1 << (lg > 40 ? 40 : lg); }();
  return v;
}
// The two half-size jobs of a split call: pc_hip_last_msm_phases_ms then reports the SUM of both jobs' phase brackets (the halves run
// one after the other on the device where it matters: two accumulations never share the chip usefully), pc_hip_last_msm_marks_ms and
// pc_hip_last_msm_shape the second job's (one set of marks cannot describe two pipelines).  A job that an enqueue already completed
// (lane reuse) contributed its phases then; they are lost to the sum -- with PC_MSM_LANES = 3 pipelines that never happens for two jobs.
static void complete_two(pc_ctx* ctx, pc_job* a, pc_job* b) {
  float ph[8] = {0};
  if (!a->done) { complete_job(ctx, a); for (int i = 0; i < 8; i++) ph[i] = ctx->phases[i]; }
  if (!b->done) { complete_job(ctx, b); for (int i = 0; i < 8; i++) ctx->phases[i] += ph[i]; }
}
// Host scalars of at least host_split_min() pairs: ONE MSM in PC_HIP_HOST_PARTS parts (default 4; 0 = the two half-size MSMs on two
// pipelines of round 4) on one pipeline -- MsmPlan::begin_parts: the copy and sort of part k + 1 run beside the accumulation of part k,
// all parts share one bucket reduction and one host tail.
// PC_HIP_HOST_PARTS: a part count (equal parts) or a comma list of relative weights (default "1,2,5,8": a short first part, so that the
// first copy and sort -- the only ones nothing hides -- are short; measured at 2^24 BLS12-381: commit of host coefficients 40.3 ms against
// 38.5 resident and 46.8 as two half-size MSMs, open 41.7 against 39.5 / 46.8; four equal parts 44.0 / 45.3, "1,3,4,8" 40.9 / 42.4).
static const std::vector<double>& host_part_cuts() {      // cumulative fractions: cuts[0] = 0 < ... < cuts[K] = 1; empty = no parts
  static const std::vector<double> cuts = []() {
    std::vector<double> w;
    const char* e = getenv("PC_HIP_HOST_PARTS");
    std::string spec = e ? e : "1,2,5,8";
    if (spec.find(',') == std::string::npos) { int k = atoi(spec.c_str()); if (k > 8) k = 8; for (int i = 0; i < k; i++) w.push_back(1.0); }
    else { size_t at = 0; while (at <= spec.size() && w.size() < 8) { size_t c = spec.find(',', at); if (c == std::string::npos) c = spec.size(); double v = atof(spec.substr(at, c - at).c_str()); if (v > 0) w.push_back(v); at = c + 1; } }
    std::vector<double> out;
    if (w.size() < 2) return out;
    double tot = 0; for (double v : w) tot += v;
    double acc = 0; out.push_back(0.0);
    for (double v : w) { acc += v; out.push_back(acc / tot); }
    out.back() = 1.0;
    return out;
  }();
  return cuts;
}
static size_t host_parts() { return host_part_cuts().empty() ? 0 : host_part_cuts().size() - 1; }
static size_t part_cut(size_t n, size_t k) { const auto& c = host_part_cuts(); return k + 1 >= c.size() ? n : (size_t)((double)n * c[k]); }
// claim a pipeline of the key for a job in `total` pairs that arrive in parts (completing what it still holds).  Always the first one: a blocking call gains nothing from
// rotating, and only the pipeline that runs parts grows the second sort output and bucket array (1.2 GB at 2^24 BLS12-381 points).
static MsmLane* begin_parts(pc_ctx* ctx, pc_srs* srs, size_t total, void* out_xy, int* out_is_infinity, pc_job* job) {
  MsmLane* L = claim_lane(ctx, srs, 0, out_xy, out_is_infinity, job);
  L->runner->begin_parts(total);
  L->inflight = job;                           // from here on the pipeline holds work of this job (the caller's StackJob completes it on any exit)
  return L;
}
// one MSM on the key's next pipeline, waited for
static int msm_blocking(pc_ctx* ctx, pc_srs* srs, size_t base_offset, const void* scalars, pc_scalar_form form, pc_mem where, size_t n,
                        void* out_xy, int* out_is_infinity) {
  pc_job job;
  int rc = enqueue_job(ctx, srs, base_offset, scalars, form, where, n, out_xy, out_is_infinity, &job);
  if (rc == PC_OK) complete_job(ctx, &job);
  return rc;
}
// sum of two affine results into out_xy / out_is_infinity
static void fold_two(pc_srs* srs, const uint32_t* a, const uint32_t* b, void* out_xy, int* out_is_infinity) {
  std::vector<uint32_t> two(2 * (size_t)srs->aw);
  memcpy(two.data(), a, (size_t)srs->aw * 4); memcpy(two.data() + srs->aw, b, (size_t)srs->aw * 4);
  pc::curve_ops(srs->curve).points_sum(two.data(), 2, (uint32_t*)out_xy);
  if (out_is_infinity) *out_is_infinity = affine_is_zero((const uint32_t*)out_xy, srs->aw);
}

extern "C" {

int pc_hip_msm(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* scalars, pc_scalar_form form,
               pc_mem where, size_t n, void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !out_xy || srs->ctx != ctx) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const size_t avail = base_offset <= srs->n ? srs->n - base_offset : 0;
    const size_t ne = n < avail ? n : avail;
    if (where == PC_MEM_HOST && scalars && ne >= host_split_min() && base_offset <= srs->n && host_parts() >= 2) {
      const size_t K = host_parts();
      StackJob j(ctx);
      MsmLane* L = begin_parts(ctx, srs, ne, out_xy, out_is_infinity, &j.job);
      std::vector<std::pair<size_t, size_t>> parts;        // (first, count), empty parts dropped
      for (size_t k = 0; k < K; k++) { const size_t first = part_cut(ne, k), cnt = part_cut(ne, k + 1) - first; if (cnt) parts.push_back({first, cnt}); }
      for (size_t k = 0; k < parts.size(); k++)
        L->runner->add_part(srs->bases, (uint32_t)base_offset, parts[k].first, (const uint8_t*)scalars + parts[k].first * 32, PC_MEM_HOST, parts[k].second,
                            form == PC_SCALARS_MONTGOMERY, k + 1 == parts.size());
      complete_job(ctx, &j.job);
      return (int)PC_OK;
    }
    if (where == PC_MEM_HOST && scalars && ne >= host_split_min() && base_offset <= srs->n) {
      const size_t h = ne / 2;
      std::vector<uint32_t> r1(srs->aw), r2(srs->aw);
      StackJob j1(ctx), j2(ctx);
      int rc = enqueue_job(ctx, srs, base_offset, scalars, form, where, h, r1.data(), nullptr, &j1.job);
      if (rc != PC_OK) return rc;
      rc = enqueue_job(ctx, srs, base_offset + h, (const uint8_t*)scalars + h * 32, form, where, ne - h, r2.data(), nullptr, &j2.job);
      if (rc != PC_OK) return rc;
      complete_two(ctx, &j1.job, &j2.job);
      fold_two(srs, r1.data(), r2.data(), out_xy, out_is_infinity);
      return (int)PC_OK;
    }
    return msm_blocking(ctx, srs, base_offset, scalars, form, where, n, out_xy, out_is_infinity);
  });
}

int pc_hip_msm_async(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* scalars, pc_scalar_form form,
                     pc_mem where, size_t n, void* out_xy, int* out_is_infinity, pc_job** out_job) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !out_xy || !out_job || srs->ctx != ctx) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  *out_job = nullptr;
  pc_job* job = new (std::nothrow) pc_job();
  if (!job) return PC_ERR_OOM;
  int rc = guarded(ctx, [&]() { return enqueue_job(ctx, srs, base_offset, scalars, form, where, n, out_xy, out_is_infinity, job); });
  if (rc != PC_OK) { delete job; return rc; }
  *out_job = job;
  return PC_OK;
}

int pc_hip_job_wait(pc_ctx* ctx, pc_job* job) {
  if (!ctx || !job) return PC_ERR_INVALID_ARG;
  // The wait for the device happens WITHOUT the context's lock: other threads (the per-device workers of pc_hip_group_*)
  // keep queueing work on this context meanwhile -- with the lock held for the whole wait a reaper serialised them behind
  // every MSM it waited for.  The bookkeeping behind it (host tail, phase times) is under the lock as before; a job that
  // another call completed in between (enqueue_job reusing its lane) is simply found done.
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!job->done && job->srs) { MsmLane* L = job->srs->lanes[job->lane]; if (L && L->inflight == job) ev = L->be.done; }
  }
  if (ev && hipSetDevice(ctx->device) == hipSuccess) (void)hipEventSynchronize(ev);      // an error surfaces in complete_job below
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  int rc = job->status;
  if (!job->done) rc = guarded(ctx, [&]() { complete_job(ctx, job); return job->status; });
  delete job;
  return rc;
}

int pc_hip_msm_batch(pc_ctx* ctx, const pc_srs* srs_c, const size_t* base_offsets, const void* const* scalars,
                     const size_t* n, size_t n_polys, pc_scalar_form form, pc_mem where, void* out_xy,
                     int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !out_xy || srs->ctx != ctx || (n_polys && (!scalars || !n))) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    // Equal-length polynomials against the window table of the key (MarlinKZG10::commit of a batch: config 3): G of them per
    // pass through ONE sort / accumulate / reduce pipeline with a bucket set each (the many-MSM machinery of
    // pc_hip_msm_many, over the key's own table).  The latency-bound reductions and the host tail are then paid once per G
    // polynomials and are wide enough to be throughput-bound; two such pipelines alternate.
    {
      // (HOST polynomials -- what MarlinKZG10::commit hands over -- take the same passes: the G polynomials of a pass are copied to a
      // staging buffer on the pipeline that will run the pass, i.e. beside the other pipeline's pass: 64 x 2^20 host polynomials cost
      // one exposed copy of 8, not 2 GiB of PCIe in front of the batch)
      bool same = n_polys >= 2 && srs->table && n[0] >= ((size_t)1 << 14) && n[0] >= srs->cfg.tbl_min_n;
      const size_t b0 = base_offsets ? base_offsets[0] : 0;
      for (size_t k = 0; same && k < n_polys; k++) same = n[k] == n[0] && (base_offsets ? base_offsets[k] : 0) == b0 && scalars[k];
      if (same && b0 <= srs->n && n[0] <= srs->n - b0) {
        static const size_t Gmax = []() { const char* e = getenv("PC_HIP_BATCH_G"); int v = e ? atoi(e) : 8; return (size_t)(v < 0 ? 0 : v); }();
        const size_t m = n[0];
        size_t G = std::min(Gmax, n_polys);
        const uint32_t sets = srs->cfg.tbl_glv ? 2u : 1u;
        const uint32_t Wd = sets * table_windows(srs, srs->cfg.tbl_c, srs->cfg.tbl_glv);      // digits per scalar
        while (G >= 2 && ((uint64_t)G * m * Wd >= (1ull << 32) || ((uint64_t)G * sets << (srs->cfg.tbl_c - 1)) >= (1ull << 31))) G /= 2;
        // HOST polynomials are staged on the device, G of them per pipeline: that copy has a budget (BATCH_STAGE_MAX per pipeline; 8 x
        // 2^24 coefficients would be 2 x 4 GiB beside the passes' own workspace).  G shrinks to fit; below two polynomials per pass
        // the call takes the per-polynomial pipeline further down, which stages one polynomial at a time.
        static const size_t BATCH_STAGE_MAX = []() { const char* e = getenv("PC_HIP_BATCH_STAGE_MAX_MB"); long v = e ? atol(e) : 1024; return (size_t)(v < 0 ? 0 : v) << 20; }();
        if (where == PC_MEM_HOST) while (G >= 2 && (uint64_t)G * m * 32 > BATCH_STAGE_MAX) G /= 2;
        if (G >= 2) {
          pc_srs::BatchMany& B = srs->bm;
          if (B.m != m || B.G != G) {
            drop_batch_many(srs);
            for (int i = 0; i < 2; i++) {
              try { B.lanes[i] = new_lane(srs->curve, G * m, srs->cfg, (uint32_t)G); }
              catch (...) { drop_batch_many(srs); throw; }
            }
            B.m = m; B.G = G;
          }
          // both staging buffers before any pass is queued: when the device cannot give them, nothing is in flight yet and the
          // call goes on through the per-polynomial pipeline instead of failing (host inputs took that road before this path existed)
          bool staged_ok = true;
          if (where == PC_MEM_HOST)
            for (int i = 0; i < 2 && staged_ok; i++)
              if (!B.stage[i]) {
                try { B.stage[i] = (uint32_t*)B.lanes[i]->be.alloc(G * m * 32); }
                catch (const std::exception&) {
                  staged_ok = false;
                  (void)hipGetLastError();
                  for (int j = 0; j < 2; j++) if (B.stage[j]) { B.lanes[j]->be.free(B.stage[j]); B.stage[j] = nullptr; }
                }
              }
          if (staged_ok) {
          key_drain(srs);                              // nothing of the single-MSM pipelines may be in flight on this key's outputs
          const size_t pb = (size_t)srs->aw * 4;
          std::vector<uint32_t> tmp[2]; tmp[0].resize(G * srs->aw); tmp[1].resize(G * srs->aw);
          size_t pending_first[2] = {0, 0}, pending_cnt[2] = {0, 0};
          // phase brackets of the passes (pc_hip_last_msm_phases_ms after a batch): [0..5] summed over the passes, [6] the union of
          // the passes' accumulate intervals (consecutive passes overlap on the two pipelines), [7] the number of passes
          float ph_sum[8] = {0}; std::vector<std::pair<float, float>> acc_iv;
          auto drain = [&](int li) {
            if (!pending_cnt[li]) return;
            B.lanes[li]->runner->finish(tmp[li].data());
            pc::HipBackend& lbe = B.lanes[li]->be;
            if (lbe.timing && lbe.n_ev >= 5) {
              for (int i = 0; i + 1 < lbe.n_ev && i < 6; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, lbe.ev[i], lbe.ev[i + 1]); ph_sum[i] += ms; }
              if (ctx->epoch) { float a = 0, b = 0; (void)hipEventElapsedTime(&a, ctx->epoch, lbe.ev[3]); (void)hipEventElapsedTime(&b, ctx->epoch, lbe.ev[4]); acc_iv.push_back({a, b}); }
              ph_sum[7] += 1.0f;
            }
            for (size_t k = 0; k < pending_cnt[li]; k++) {
              uint8_t* o = (uint8_t*)out_xy + (pending_first[li] + k) * pb;
              memcpy(o, tmp[li].data() + k * srs->aw, pb);
              if (out_is_infinity) out_is_infinity[pending_first[li] + k] = affine_is_zero(tmp[li].data() + k * srs->aw, srs->aw);
            }
            pending_cnt[li] = 0;
          };
          int li = 0;
          for (size_t first = 0; first < n_polys; first += G, li ^= 1) {
            drain(li);
            const size_t cnt = std::min(G, n_polys - first);
            std::vector<uint64_t> ptrs(cnt);
            if (where == PC_MEM_HOST) {
              pc::HipBackend& lbe = B.lanes[li]->be;
              for (size_t k = 0; k < cnt; k++) {
                uint32_t* dst = B.stage[li] + k * m * 8;
                lbe.copy_h2d(dst, scalars[first + k], m * 32);
                ptrs[k] = (uint64_t)(uintptr_t)dst;
              }
            } else
              for (size_t k = 0; k < cnt; k++) ptrs[k] = (uint64_t)(uintptr_t)scalars[first + k];
            B.lanes[li]->be.timing = ctx->be.timing;
            B.lanes[li]->runner->enqueue_vectors(srs->bases, (uint32_t)b0, ptrs.data(), cnt, m, form == PC_SCALARS_MONTGOMERY);
            pending_first[li] = first; pending_cnt[li] = cnt;
          }
          drain(li); drain(li ^ 1);
          if (ctx->be.timing) {
            std::sort(acc_iv.begin(), acc_iv.end());
            float tot = 0, end = -1e30f;
            for (auto& iv : acc_iv) { if (iv.second <= end) continue; tot += iv.second - std::max(iv.first, end); end = iv.second; }
            ph_sum[6] = tot;
            for (int i = 0; i < 8; i++) ctx->phases[i] = ph_sum[i];
            B.lanes[0]->runner->shape(ctx->shape);
          }
          // staging above the keep threshold is transient, as the single-call buffers are (CallBuf / STAGE_KEEP)
          static constexpr size_t BATCH_STAGE_KEEP = (size_t)256 << 20;
          if (where == PC_MEM_HOST && G * m * 32 > BATCH_STAGE_KEEP)
            for (int i = 0; i < 2; i++) if (B.stage[i]) { B.lanes[i]->be.free(B.stage[i]); B.stage[i] = nullptr; }
          return (int)PC_OK;
          }      // staged_ok
        }
      }
    }
    // software pipeline over the lanes: polynomial k+1 accumulates while k's tail drains
    std::vector<pc_job> jobs(n_polys);
    for (size_t k = 0; k < n_polys; k++) {
      int rc = enqueue_job(ctx, srs, base_offsets ? base_offsets[k] : 0, scalars[k], form, where, n[k],
                           (uint8_t*)out_xy + k * (size_t)srs->aw * 4, out_is_infinity ? out_is_infinity + k : nullptr, &jobs[k]);
      if (rc != PC_OK) { for (size_t j = 0; j < k; j++) if (!jobs[j].done) complete_job(ctx, &jobs[j]); return rc; }
    }
    for (size_t k = 0; k < n_polys; k++) if (!jobs[k].done) complete_job(ctx, &jobs[k]);
    return (int)PC_OK;
  });
}

int pc_hip_msm_many(pc_ctx* ctx, pc_srs* srs, size_t base_offset, const void* scalars, pc_scalar_form form, pc_mem where,
                    size_t m, size_t n_msms, void* out_xy, int* out_is_infinity) {
  if (!ctx || !srs || srs->ctx != ctx || !out_xy || (m && n_msms && !scalars)) return PC_ERR_INVALID_ARG;
  if (base_offset > srs->n || m > srs->n - base_offset) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const size_t pb = (size_t)srs->aw * 4;
    if (!n_msms) return (int)PC_OK;
    if (!m) { memset(out_xy, 0, n_msms * pb); if (out_is_infinity) for (size_t k = 0; k < n_msms; k++) out_is_infinity[k] = 1; return (int)PC_OK; }
    const uint32_t bits = pc::curve_ops(srs->curve).scalar_bits;      // 255 / 254 / 255 / 253
    const uint32_t c = pc::msm_choose_table_c(m, bits, 0), Wd = pc::msm_num_windows(bits, c);
    if ((uint64_t)n_msms * m * Wd >= (1ull << 31) || ((uint64_t)n_msms << (c - 1)) >= (1ull << 31)) return (int)PC_ERR_TOO_LARGE;
    pc_srs::Many& M = srs->many;
    if (!M.lane || M.base_offset != base_offset || M.m != m || M.B != n_msms) {
      drop_many(srs);
      uint32_t* table = (uint32_t*)ctx->be.alloc((size_t)Wd * m * pb);
      MsmLane* L = nullptr;
      try {
        const uint32_t* b0 = srs->bases + base_offset * srs->aw;
        pc::curve_ops(srs->curve).window_table(ctx->be, b0, (uint32_t)m, c, Wd, table, (uint32_t)srs->aw);
        pc::MsmConfig cfg = srs->cfg;
        cfg.c = 0; cfg.T = 0; cfg.tbl = table; cfg.tbl_c = c; cfg.tbl_stride = (uint32_t)m; cfg.tbl_pt_stride = (uint32_t)srs->aw; cfg.tbl_min_n = 0;
        cfg.tbl_glv = false;      // this pass's own table is the full one: c, Wd and the capacity checks above are the plain form's, whatever the key's table is
        L = new_lane(srs->curve, n_msms * m, cfg, (uint32_t)n_msms);
      } catch (...) { ctx->be.free(table); throw; }
      M.table = table; M.lane = L; M.base_offset = base_offset; M.m = m; M.B = n_msms;
    }
    MsmLane* L = M.lane;
    L->be.timing = ctx->be.timing;
    L->runner->enqueue(srs->bases, 0, scalars, where, n_msms * m, form == PC_SCALARS_MONTGOMERY);
    L->runner->finish((uint32_t*)out_xy);
    if (out_is_infinity) {
      const uint32_t* o = (const uint32_t*)out_xy;
      for (size_t k = 0; k < n_msms; k++) out_is_infinity[k] = affine_is_zero(o + k * srs->aw, srs->aw);
    }
    lane_phases(ctx, L);
    return (int)PC_OK;
  });
}

int pc_hip_points_sum(pc_curve curve, const void* points_xy, size_t count, void* out_xy) {
  if (!pc_known_curve(curve) || !out_xy || (count && !points_xy)) return PC_ERR_INVALID_ARG;
  pc::curve_ops(curve).points_sum((const uint32_t*)points_xy, count, (uint32_t*)out_xy);
  return PC_OK;
}

// KZG10::open without hiding (poly-commit/src/kzg10/mod.rs:287-310: compute_witness_polynomial :217-240, then
// open_with_witness_polynomial's MSM :255-258) as ONE call: W = sum_j q[j] * powers[base_offset + j], q = p / (x - z).
// The quotient never leaves the device.  Host coefficients of at least host_split_min() elements run in parts, top part first (its
// quotient needs nothing from below): copy + division of a part on the context's queue beside the accumulation of the part above on
// the key's pipeline, every further division with the carry q[hi] of the part above; ONE MSM over all parts (MsmPlan::begin_parts).
int pc_hip_kzg_open(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, const void* coeffs, pc_mem where, size_t n, const void* z_host,
                    void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || srs->ctx != ctx || !out_xy || !z_host || (n && !coeffs)) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  if (base_offset > srs->n || (n > 1 && n - 1 > srs->n - base_offset)) return PC_ERR_INVALID_ARG;     // the reference checks the degree before (kzg10/mod.rs:393-407)
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n <= 1) { memset(out_xy, 0, (size_t)srs->aw * 4); if (out_is_infinity) *out_is_infinity = 1; return (int)PC_OK; }
    const pc::FieldOps& F = pc::field_ops(srs->curve);
    const uint32_t* z = (const uint32_t*)z_host;
    const size_t m = n - 1;                                       // quotient length; x[j] = p[j + 1]
    // the quotient (and, in the split path, the shifted coefficients): the context's grow-only staging up to STAGE_KEEP, transient
    // buffers above it -- one open of a 2^26-coefficient polynomial would otherwise pin 2 x 2 GiB until pc_hip_ctx_trim.  The transient
    // ones are freed when the call returns: every job that reads them is complete by then (StackJob / complete_job below).
    CallBuf qbuf(ctx->be, 1, m * 32);
    uint32_t* q = (uint32_t*)qbuf.dev;
    if (where == PC_MEM_DEVICE || n < host_split_min()) {
      Staged sin(ctx->be, coeffs, where, n * 32, true, 0);
      F.witness(ctx->be, (const uint32_t*)sin.dev, n, z, q, scan_fan());
      return msm_blocking(ctx, srs, base_offset, q, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, m, out_xy, out_is_infinity);
    }
    CallBuf xbuf(ctx->be, 0, m * 32);
    uint32_t* x = (uint32_t*)xbuf.dev;
    const uint8_t* src = (const uint8_t*)coeffs + 32;
    if (host_parts() >= 2) {
      // the quotient in parts, TOP part first (its scan needs nothing from below; every further part takes the carry q[hi] of the one
      // above): copy + division of part t + 1 on the context's queue beside the accumulation of part t on the key's pipeline; one MSM
      const size_t K = host_parts();
      std::vector<uint32_t> carry(8);
      StackJob j(ctx);
      MsmLane* L = begin_parts(ctx, srs, m, out_xy, out_is_infinity, &j.job);
      std::vector<std::pair<size_t, size_t>> parts;        // (lo, hi) from the top; part t of the weights counted from the top
      for (size_t t = 0; t < K; t++) { const size_t hi = m - part_cut(m, t), lo = m - part_cut(m, t + 1); if (hi > lo) parts.push_back({lo, hi}); }
      for (size_t t = 0; t < parts.size(); t++) {
        const size_t lo = parts[t].first, hi = parts[t].second, len = hi - lo;
        ctx->be.copy_h2d(x + lo * 8, src + lo * 32, len * 32);
        if (t) ctx->be.copy_d2h(carry.data(), q + hi * 8, 32);
        F.div_scan(ctx->be, x + lo * 8, len, z, t ? carry.data() : nullptr, q + lo * 8, scan_fan());      // (returns with the stream drained)
        L->runner->add_part(srs->bases, (uint32_t)base_offset, lo, q + lo * 8, PC_MEM_DEVICE, len, true, t + 1 == parts.size());
      }
      complete_job(ctx, &j.job);
      return (int)PC_OK;
    }
    const size_t h = m / 2;
    std::vector<uint32_t> r1(srs->aw), r2(srs->aw), carry(8);
    StackJob j1(ctx), j2(ctx);
    ctx->be.copy_h2d(x + h * 8, src + h * 32, (m - h) * 32);
    F.div_scan(ctx->be, x + h * 8, m - h, z, nullptr, q + h * 8, scan_fan());          // (returns with the stream drained)
    int rc = enqueue_job(ctx, srs, base_offset + h, q + h * 8, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, m - h, r1.data(), nullptr, &j1.job);
    if (rc != PC_OK) return rc;
    ctx->be.copy_h2d(x, src, h * 32);
    ctx->be.copy_d2h(carry.data(), q + h * 8, 32);
    F.div_scan(ctx->be, x, h, z, carry.data(), q, scan_fan());
    rc = enqueue_job(ctx, srs, base_offset, q, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, h, r2.data(), nullptr, &j2.job);
    if (rc != PC_OK) return rc;
    complete_two(ctx, &j1.job, &j2.job);
    fold_two(srs, r1.data(), r2.data(), out_xy, out_is_infinity);
    return (int)PC_OK;
  });
}

}  // extern "C"
