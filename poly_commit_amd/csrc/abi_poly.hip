// C ABI of the gfx950 backend (include/pc_hip.h): polynomial kernels, NTT, hashing, Merkle tree, Ligero commit.
#include <chrono>
#include <condition_variable>
#include <thread>
#include <stdio.h>
#include <string.h>
#include "abi_fr.hpp"

using pc::NttRunner;

// the context's NTT plan of 2^log_n points over one field, made on first use
static NttRunner* ntt_plan(pc_ctx* ctx, pc_curve field_of, unsigned log_n) {
  auto& plan = ctx->ntt_plans[std::make_pair((int)field_of, log_n)];
  if (!plan) plan.reset(pc::field_ops(field_of).make_ntt(ctx->be, log_n));
  return plan.get();
}

// pc_hip_ligero_commit with the matrix AND the encoded matrix on the host (what LinearCodePCS::commit hands over and keeps,
// linear_codes/mod.rs:248-268): the encoded matrix is 2^log_n / in_cols times the input and its way back over PCIe is the longest
// leg of the call by far (config 5: 2 GiB, ~37 ms, against 9 ms in and 7 ms of kernels).  The rows are independent
// (compute_matrices, mod.rs:131-135) and the column digests chain over row slabs (pc_hip_column_hash_part), so the call runs in slabs of
// consecutive rows: slab s is copied in and encoded + absorbed on the context's queue while helper threads copy the slabs before it
// out on queues of their own.  helpers + 1 slab buffers each way instead of the whole encoded matrix in HBM.
//
// The caller's matrices are pageable memory, and a pageable copy blocks its calling thread while the runtime pins the pages (or finds
// them in its cache of recent pins), moves them by DMA and lets go of them.  With ONE helper the call took 41 ms as long as that cache
// hit -- the same buffers call after call in a quiet process -- and 80-82 ms whenever it did not (measured: from the moment a key with
// its tables had been freed, for as long as the probe ran): pinning and unpinning 2 GiB costs about as much host time as moving them
// takes, and one thread does the two one after the other.  So several helpers take the slabs in turn, one pinning while another's
// DMA runs (after a key was freed: 82 / 53 / 43-46 / 52 ms with 1 / 2 / 3 / 4 helpers; quiet: 40-42 ms with any).  The way IN stays with
// the runtime too: with one helper it was the slow side after a key was freed (a bounce-buffer memcpy at 11 GB/s of the calling
// thread), with three it hides under the way out, and registering the coefficient matrix's pages from the calling thread instead
// (page-aligned pieces just ahead of the copies, released behind them: built in round 5 as PC_HIP_LIGERO_PIN=1) measured 2-3 ms slower in
// both states (42.3 vs 40.0 ms quiet, 46.0 vs 42.8 ms after a key was freed: releasing a registration waits for the device) and was
// REMOVED in round 6: the library maps no caller memory into the device's address space (EXPERIMENTS 00).
// The whole-matrix path of the same call: 58-60 ms in either state.
// PC_HIP_LIGERO_SLAB_MB: encoded bytes per slab (default 32; 0 = the whole-matrix path), PC_HIP_LIGERO_HELPERS (default 3, at most 4),
// PC_HIP_LIGERO_TRACE=1: where the threads spent the call, on stderr;
// all read per call.  tools/ligero_stream_probe.py sweeps them in both states of the process.
static constexpr int LIG_MAX_HELPERS = 4;
// the Merkle tree's nodes (2^h - 1 of them over the padded leaf count 2^h >= 2) and, on request, the leaves to the host
static void ligero_download(pc_ctx* ctx, size_t N, const void* nodes, const void* leaves, void* nodes_out_host, void* leaves_out_host) {
  unsigned h = 1; while (((size_t)1 << h) < N) h++;
  ctx->be.copy_d2h(nodes_out_host, nodes, (((size_t)1 << h) - 1) * 32);
  if (leaves_out_host) ctx->be.copy_d2h(leaves_out_host, leaves, N * 32);
}
static int lig_helpers() { const char* e = getenv("PC_HIP_LIGERO_HELPERS"); const int h = e ? atoi(e) : 3; return h < 1 ? 1 : h > LIG_MAX_HELPERS ? LIG_MAX_HELPERS : h; }
static size_t ligero_slab_rows(size_t rows, size_t N) {
  const char* e = getenv("PC_HIP_LIGERO_SLAB_MB");
  const double mb = e ? atof(e) : 32.0;
  if (!(mb > 0)) return 0;
  size_t s = (size_t)(mb * 1048576.0 / ((double)N * 32.0));
  s &= ~(size_t)1;                                     // every slab but the last holds an even number of rows (two rows fill a block)
  if (s < 2) s = 2;
  return s * 2 <= rows ? s : 0;                        // fewer than two slabs: nothing to overlap
}

static int ligero_commit_streamed(pc_ctx* ctx, pc_curve field_of, const char* mat, size_t rows, size_t in_cols, unsigned log_n, size_t S,
                                  pc_hash col_hash, pc_hash tree_hash, int len_prefix, char* ext_out, void* leaves_out_host, void* nodes_out_host) {
  const size_t N = (size_t)1 << log_n, n_slabs = (rows + S - 1) / S;
  const size_t in_row = in_cols * 32, ext_row = N * 32;
  const bool with_digests = nodes_out_host != nullptr;      // pc_hip_ntt_batch host -> host takes the same road without them
  const int LIG_HELPERS = lig_helpers(), LIG_BUFS = LIG_HELPERS + 1;      // one slab under the kernels, one with every helper
  void* in_dev[LIG_MAX_HELPERS + 1] = {}; void* ext_dev[LIG_MAX_HELPERS + 1] = {};
  void* state = nullptr; void* leaves = nullptr; void* nodes = nullptr; void* transient = nullptr;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t a_in = up(S * in_row), a_ext = up(S * ext_row), a_state = up(N * 48), a_leaves = up(N * 32), a_nodes = up((N > 1 ? N : 2) * 32);
  const size_t arena_bytes = LIG_BUFS * (a_in + a_ext) + a_state + a_leaves + a_nodes;
  static constexpr size_t LIGERO_KEEP = (size_t)512 << 20;
  std::vector<hipEvent_t> done(n_slabs, nullptr);
  // caller -> helpers: slabs whose kernels are queued (their event is recorded); helpers -> caller: slabs that have arrived
  std::mutex mu; std::condition_variable cv;
  size_t queued = 0; std::vector<char> arrived(n_slabs, 0); bool stop = false; int helper_rc = PC_OK; std::string helper_err;
  std::thread helpers[LIG_MAX_HELPERS];
  double tr_out[LIG_MAX_HELPERS] = {}, tr_in[3] = {0, 0, 0};      // PC_HIP_LIGERO_TRACE: helpers [copies out], caller [input buffer free, pin + copy in, slab buffer free]
  auto now_ms = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  int rc = guarded(ctx, [&]() {
    char* a;
    if (arena_bytes <= LIGERO_KEEP) {
      if (arena_bytes > ctx->lig_bytes) {
        ctx->be.sync(); ctx->be.free(ctx->lig_arena); ctx->lig_arena = nullptr; ctx->lig_bytes = 0;
        ctx->lig_arena = ctx->be.alloc(arena_bytes); ctx->lig_bytes = arena_bytes;
      }
      a = (char*)ctx->lig_arena;
    } else {
      a = (char*)(transient = ctx->be.alloc(arena_bytes));
    }
    for (int b = 0; b < LIG_BUFS; b++) { in_dev[b] = a; a += a_in; ext_dev[b] = a; a += a_ext; }
    state = a; a += a_state; leaves = a; a += a_leaves; nodes = a;
    for (int h = 0; h < LIG_HELPERS; h++)
      if (!ctx->lig_out_q[h]) PC_HIP_CHECK(hipStreamCreateWithFlags(&ctx->lig_out_q[h], hipStreamNonBlocking));
    for (auto& e : done) PC_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    NttRunner* ntt = ntt_plan(ctx, field_of, log_n);
    for (int h = 0; h < LIG_HELPERS; h++)
      helpers[h] = std::thread([&, h]() {
        try {
          PC_HIP_CHECK(hipSetDevice(ctx->device));
          hipStream_t q = ctx->lig_out_q[h];
          for (size_t s = (size_t)h; s < n_slabs; s += LIG_HELPERS) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return queued > s || stop; }); if (queued <= s) return; }
            const size_t r0 = s * S, nr = std::min(S, rows - r0);
            const double t_a = now_ms();
            PC_HIP_CHECK(hipStreamWaitEvent(q, done[s], 0));
            PC_HIP_CHECK(hipMemcpyAsync(ext_out + r0 * ext_row, ext_dev[s % LIG_BUFS], nr * ext_row, hipMemcpyDeviceToHost, q));
            PC_HIP_CHECK(hipStreamSynchronize(q));
            tr_out[h] += now_ms() - t_a;
            { std::lock_guard<std::mutex> lk(mu); arrived[s] = 1; }
            cv.notify_all();
          }
        } catch (const std::exception& e) {
          { std::lock_guard<std::mutex> lk(mu); helper_rc = PC_ERR_HIP; helper_err = e.what(); std::fill(arrived.begin(), arrived.end(), 1); }   // releases the caller
          cv.notify_all();
        }
      });
    const bool marks = ctx->be.timing_marks(false);
    struct Restore { pc::HipBackend& be; bool m; ~Restore() { be.timing_marks(m); } } restore{ctx->be, marks};
    for (size_t s = 0; s < n_slabs; s++) {
      const int b = (int)(s % LIG_BUFS);
      const size_t r0 = s * S, nr = std::min(S, rows - r0);
      const double t_a = now_ms();
      if (s >= (size_t)LIG_BUFS) PC_HIP_CHECK(hipEventSynchronize(done[s - LIG_BUFS]));        // in_dev[b] has been read
      const double t_b = now_ms();
      {
        ctx->be.copy_h2d(in_dev[b], mat + r0 * in_row, nr * in_row);
      }
      const double t_c = now_ms();
      if (s >= (size_t)LIG_BUFS) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return arrived[s - LIG_BUFS] != 0; }); }   // ext_dev[b] is on the host
      tr_in[0] += t_b - t_a; tr_in[1] += t_c - t_b; tr_in[2] += now_ms() - t_c;
      { std::lock_guard<std::mutex> lk(mu); if (helper_rc != PC_OK) break; }
      ntt->run((const uint32_t*)in_dev[b], nr, in_cols, (uint32_t*)ext_dev[b]);
      if (with_digests)
        pc::field_ops(field_of).column_hash_part(ctx->be, (int)col_hash, (const uint32_t*)ext_dev[b], (uint32_t)nr, (uint32_t)N, (uint32_t)rows, 0u,
                                                 (uint32_t)N, s == 0, s + 1 == n_slabs, (uint32_t*)state, (uint32_t*)leaves);
      PC_HIP_CHECK(hipEventRecord(done[s], ctx->be.stream));
      { std::lock_guard<std::mutex> lk(mu); queued = s + 1; }
      cv.notify_all();
    }
    return (int)PC_OK;
  });
  if (rc == PC_OK && helper_rc == PC_OK && with_digests) {      // the tree and the small downloads run beside the last slabs' way out
    rc = pc_hip_merkle_tree(ctx, tree_hash, leaves, PC_MEM_DEVICE, N, len_prefix, nodes, PC_MEM_DEVICE);
    if (rc == PC_OK) rc = guarded(ctx, [&]() {
      ligero_download(ctx, N, nodes, leaves, nodes_out_host, leaves_out_host);
      return (int)PC_OK;
    });
  }
  { std::lock_guard<std::mutex> lk(mu); stop = true; }
  cv.notify_all();
  for (auto& t : helpers) if (t.joinable()) t.join();
  if (rc == PC_OK && helper_rc != PC_OK) { ctx->last_error = helper_err; rc = helper_rc; }
  (void)guarded(ctx, [&]() {
    (void)hipStreamSynchronize(ctx->be.stream);
    for (int h = 0; h < LIG_HELPERS; h++) if (ctx->lig_out_q[h]) (void)hipStreamSynchronize(ctx->lig_out_q[h]);
    ctx->be.free(transient);
    for (auto e : done) if (e) (void)hipEventDestroy(e);
    return (int)PC_OK;
  });
  if (getenv("PC_HIP_LIGERO_TRACE"))
    fprintf(stderr, "[pc_hip] ligero slabs %zu x %zu rows: helpers' copies out %.1f / %.1f ms | caller in-buffer %.1f copy in %.1f out-buffer %.1f ms\n",
            n_slabs, S, tr_out[0], tr_out[LIG_HELPERS - 1], tr_in[0], tr_in[1], tr_in[2]);
  const float ph[4] = {0, 0, 0, with_digests ? ctx->ntt_phases[0] : 0.f};      // the slabs' kernels overlap the copies: only the tree has a bracket of its own
  memcpy(ctx->ligero_phases, ph, sizeof ph);
  return rc;
}

extern "C" {

int pc_hip_ntt_batch(pc_ctx* ctx, pc_curve field_of, const void* in, pc_mem where_in, size_t rows, size_t in_cols,
                     unsigned log_n, void* out, pc_mem where_out) {
  if (!ctx || !pc_known_curve(field_of) || (rows && (!in || !out))) return PC_ERR_INVALID_ARG;
  const unsigned max_lg = field_of == PC_CURVE_BN254 ? 28 : 32;      // BN254: the two-adicity; the others (32, 32, 47): the 32-bit indices
  if (log_n > max_lg) return PC_ERR_TOO_LARGE;
  if (log_n > PC_HIP_NTT_MAX_LOG_N) return PC_ERR_UNSUPPORTED;   // two LDS-staged passes: one factor must fit the 160 KB LDS
  if (in_cols > ((size_t)1 << log_n)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  // host -> host (LinearEncode::encode over a whole matrix, the shim's encode_matrix): in slabs of rows, the encoded slabs on their way
  // back beside the kernels of the next ones -- pc_hip_ligero_commit's road without the digests
  if (where_in == PC_MEM_HOST && where_out == PC_MEM_HOST && rows && in_cols && rows < (1ull << 32))
    if (const size_t S = ligero_slab_rows(rows, (size_t)1 << log_n)) {
      ctx->ntt_phases[0] = ctx->ntt_phases[1] = 0;
      return ligero_commit_streamed(ctx, field_of, (const char*)in, rows, in_cols, log_n, S, PC_HASH_SHA256, PC_HASH_SHA256, 0, (char*)out, nullptr, nullptr);
    }
  return guarded(ctx, [&]() {
    if (rows == 0) return (int)PC_OK;
    NttRunner* ntt = ntt_plan(ctx, field_of, log_n);
    const size_t N = (size_t)1 << log_n;
    Staged sin(ctx->be, in, where_in, rows * in_cols * 32, true, 0);
    Staged sout(ctx->be, out, where_out, rows * N * 32, false, 1);
    ctx->be.n_ev = 0;
    ntt->run((const uint32_t*)sin.dev, rows, in_cols, (uint32_t*)sout.dev);
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, rows * N * 32); else ctx->be.sync();
    ctx->ntt_phases[0] = ctx->ntt_phases[1] = 0;
    if (ctx->be.timing && ctx->be.n_ev >= 3) {
      (void)hipEventElapsedTime(&ctx->ntt_phases[0], ctx->be.ev[0], ctx->be.ev[1]);
      (void)hipEventElapsedTime(&ctx->ntt_phases[1], ctx->be.ev[1], ctx->be.ev[2]);
    }
    return (int)PC_OK;
  });
}

int pc_hip_last_ntt_phases_ms(const pc_ctx* ctx, float out[2]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  out[0] = ctx->ntt_phases[0]; out[1] = ctx->ntt_phases[1];
  return PC_OK;
}

int pc_hip_poly_eval(pc_ctx* ctx, pc_curve field_of, const void* coeffs, pc_mem where_in, size_t n, const void* z_host,
                     void* out_host) {
  if (!ctx || !pc_known_curve(field_of) || !z_host || !out_host || (n && !coeffs)) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sin(ctx->be, coeffs, where_in, n * 32, true, 0);
    const uint32_t* z = (const uint32_t*)z_host;
    pc::field_ops(field_of).poly_eval(ctx->be, (const uint32_t*)sin.dev, n, z, (uint32_t*)out_host, scan_fan());
    return (int)PC_OK;
  });
}

int pc_hip_poly_div_scan(pc_ctx* ctx, pc_curve field_of, const void* coeffs, pc_mem where_in, size_t n, const void* z_host,
                         const void* carry_in_host, void* out, pc_mem where_out) {
  if (!ctx || !pc_known_curve(field_of) || !z_host || (n && (!coeffs || !out))) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n == 0) return (int)PC_OK;
    Staged sin(ctx->be, coeffs, where_in, n * 32, true, 0);
    Staged sout(ctx->be, out, where_out, n * 32, false, 1);
    const uint32_t* z = (const uint32_t*)z_host; const uint32_t* cin = (const uint32_t*)carry_in_host;
    pc::field_ops(field_of).div_scan(ctx->be, (const uint32_t*)sin.dev, n, z, cin, (uint32_t*)sout.dev, scan_fan());
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, n * 32);
    return (int)PC_OK;
  });
}

int pc_hip_column_hash(pc_ctx* ctx, pc_curve field_of, const void* ext_mat, pc_mem where_in, size_t rows, size_t n_cols,
                       pc_hash hash, void* out_digests, pc_mem where_out) {
  if (!ctx || !pc_known_curve(field_of) || ((int)hash != PC_HASH_SHA256 && (int)hash != PC_HASH_BLAKE2S) ||
      (rows && n_cols && (!ext_mat || !out_digests))) return PC_ERR_INVALID_ARG;
  if (rows >= (1ull << 32) || n_cols >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!n_cols) return (int)PC_OK;
    Staged sin(ctx->be, ext_mat, where_in, rows * n_cols * 32, true, 0);
    Staged sout(ctx->be, out_digests, where_out, n_cols * 32, false, 1);
    const uint32_t* e = (const uint32_t*)sin.dev; uint32_t* o = (uint32_t*)sout.dev;
    ctx->be.n_ev = 0; ctx->be.mark();
    pc::field_ops(field_of).column_hash(ctx->be, (int)hash, e, (uint32_t)rows, (uint32_t)n_cols, o);
    ctx->be.mark();
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out_digests, sout.dev, n_cols * 32); else ctx->be.sync();
    one_bracket(ctx);
    return (int)PC_OK;
  });
}

int pc_hip_column_hash_part(pc_ctx* ctx, pc_curve field_of, pc_hash hash, const void* ext_slab_dev, size_t rows, size_t n_cols, size_t rows_total,
                            size_t col0, size_t cols, int first, int last, void* state_dev, void* out_digests_dev) {
  if (!ctx || !pc_known_curve(field_of) || ((int)hash != PC_HASH_SHA256 && (int)hash != PC_HASH_BLAKE2S)) return PC_ERR_INVALID_ARG;
  if (rows >= (1ull << 32) || n_cols >= (1ull << 32) || rows_total >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  if (col0 > n_cols || cols > n_cols - col0 || rows > rows_total || (rows && cols && !ext_slab_dev)) return PC_ERR_INVALID_ARG;
  if (cols && ((!(first && last) && !state_dev) || (last && !out_digests_dev))) return PC_ERR_INVALID_ARG;
  if (!last && (rows & 1)) return PC_ERR_UNSUPPORTED;             // two rows fill one block: only the last slab may be odd
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!cols) return (int)PC_OK;
    pc::field_ops(field_of).column_hash_part(ctx->be, (int)hash, (const uint32_t*)ext_slab_dev, (uint32_t)rows, (uint32_t)n_cols, (uint32_t)rows_total,
                                             (uint32_t)col0, (uint32_t)cols, first, last, (uint32_t*)state_dev, (uint32_t*)out_digests_dev);
    ctx->be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_witness_poly(pc_ctx* ctx, pc_curve field_of, const void* coeffs, pc_mem where_in, size_t n, const void* z_host,
                        void* out, pc_mem where_out) {
  if (!ctx || !pc_known_curve(field_of) || !z_host || (n && !coeffs) || (n > 1 && !out)) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (n <= 1) return (int)PC_OK;
    Staged sin(ctx->be, coeffs, where_in, n * 32, true, 0);
    Staged sout(ctx->be, out, where_out, (n - 1) * 32, false, 1);
    const uint32_t* z = (const uint32_t*)z_host;
    pc::field_ops(field_of).witness(ctx->be, (const uint32_t*)sin.dev, n, z, (uint32_t*)sout.dev, scan_fan());
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, (n - 1) * 32);
    return (int)PC_OK;
  });
}

int pc_hip_ligero_commit(pc_ctx* ctx, pc_curve field_of, const void* mat, pc_mem where_in, size_t rows, size_t in_cols,
                         unsigned log_n, pc_hash col_hash, pc_hash tree_hash, int len_prefix, void* ext_out,
                         pc_mem where_ext, void* leaves_out_host, void* nodes_out_host) {
  if (!ctx || !rows || !in_cols || !mat || !nodes_out_host || log_n > 32 || in_cols > ((size_t)1 << log_n))
    return PC_ERR_INVALID_ARG;
  if (log_n > PC_HIP_NTT_MAX_LOG_N) return PC_ERR_UNSUPPORTED;
  auto known = [](pc_hash h) { return (int)h == PC_HASH_SHA256 || (int)h == PC_HASH_BLAKE2S; };
  if (!pc_known_curve(field_of) || !known(col_hash) || !known(tree_hash)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  const size_t N = (size_t)1 << log_n;
  if (where_in == PC_MEM_HOST && ext_out && where_ext == PC_MEM_HOST && rows < (1ull << 32))
    if (const size_t S = ligero_slab_rows(rows, N))
      return ligero_commit_streamed(ctx, field_of, (const char*)mat, rows, in_cols, log_n, S, col_hash, tree_hash, len_prefix, (char*)ext_out,
                                    leaves_out_host, nodes_out_host);
  void* ext = nullptr; void* leaves = nullptr; void* nodes = nullptr;
  const bool own_ext = !(ext_out && where_ext == PC_MEM_DEVICE);
  int rc = guarded(ctx, [&]() {
    ext = own_ext ? ctx->be.alloc(rows * N * 32) : ext_out;
    leaves = ctx->be.alloc(N * 32);
    nodes = ctx->be.alloc((N > 1 ? N : 2) * 32);
    return (int)PC_OK;
  });
  float ph[4] = {0, 0, 0, 0};
  if (rc == PC_OK) rc = pc_hip_ntt_batch(ctx, field_of, mat, where_in, rows, in_cols, log_n, ext, PC_MEM_DEVICE);
  if (rc == PC_OK) { ph[0] = ctx->ntt_phases[0]; ph[1] = ctx->ntt_phases[1]; }
  if (rc == PC_OK) rc = pc_hip_column_hash(ctx, field_of, ext, PC_MEM_DEVICE, rows, N, col_hash, leaves, PC_MEM_DEVICE);
  if (rc == PC_OK) ph[2] = ctx->ntt_phases[0];
  if (rc == PC_OK) rc = pc_hip_merkle_tree(ctx, tree_hash, leaves, PC_MEM_DEVICE, N, len_prefix, nodes, PC_MEM_DEVICE);
  if (rc == PC_OK) ph[3] = ctx->ntt_phases[0];
  if (rc == PC_OK) rc = guarded(ctx, [&]() {
    ligero_download(ctx, N, nodes, leaves, nodes_out_host, leaves_out_host);
    if (ext_out && where_ext == PC_MEM_HOST) ctx->be.copy_d2h(ext_out, ext, rows * N * 32);
    return (int)PC_OK;
  });
  (void)guarded(ctx, [&]() {
    if (own_ext && ext) ctx->be.free(ext);
    if (leaves) ctx->be.free(leaves);
    if (nodes) ctx->be.free(nodes);
    return (int)PC_OK;
  });
  memcpy(ctx->ligero_phases, ph, sizeof ph);
  return rc;
}
int pc_hip_last_ligero_phases_ms(const pc_ctx* ctx, float out[4]) {
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  memcpy(out, ctx->ligero_phases, sizeof ctx->ligero_phases);
  return PC_OK;
}

int pc_hip_merkle_tree(pc_ctx* ctx, pc_hash hash, const void* leaf_digests, pc_mem where_in, size_t n_leaves,
                       int len_prefix, void* out_nodes, pc_mem where_out) {
  if (!ctx || ((int)hash != PC_HASH_SHA256 && (int)hash != PC_HASH_BLAKE2S) || !n_leaves || !leaf_digests || !out_nodes)
    return PC_ERR_INVALID_ARG;
  if (n_leaves > (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    unsigned h = 1; while (((size_t)1 << h) < n_leaves) h++;      // padded leaf count 2^h >= 2
    const size_t n_nodes = ((size_t)1 << h) - 1;
    Staged sin(ctx->be, leaf_digests, where_in, n_leaves * 32, true, 0);
    Staged sout(ctx->be, out_nodes, where_out, n_nodes * 32, false, 1);
    uint32_t* nodes = (uint32_t*)sout.dev;
    ctx->be.n_ev = 0; ctx->be.mark();
    for (int d = (int)h - 1; d >= 0; d--) {
      const bool bottom = d == (int)h - 1;
      const size_t cnt = (size_t)1 << d;
      const uint32_t* child = bottom ? (const uint32_t*)sin.dev : nodes + (((size_t)2 << d) - 1) * 8;
      uint32_t* parent = nodes + (cnt - 1) * 8;
      pc::merkle_level(ctx->be, (int)hash, child, parent, (uint32_t)n_leaves, bottom ? 1u : 0u, len_prefix ? 1u : 0u, cnt);
    }
    ctx->be.mark();
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out_nodes, sout.dev, n_nodes * 32); else ctx->be.sync();
    one_bracket(ctx);
    return (int)PC_OK;
  });
}

int pc_hip_matrix_columns(pc_ctx* ctx, const void* mat_dev, size_t rows, size_t n_cols, const uint32_t* indices_host, size_t t,
                          void* out, pc_mem where_out) {
  if (!ctx || !mat_dev || !rows || !n_cols || (t && (!indices_host || !out))) return PC_ERR_INVALID_ARG;
  if (rows * (uint64_t)t >= (1ull << 31) || n_cols >= (1ull << 32)) return PC_ERR_TOO_LARGE;
  for (size_t j = 0; j < t; j++) if (indices_host[j] >= n_cols) return PC_ERR_INVALID_ARG;
  if (!t) return PC_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sidx(ctx->be, indices_host, PC_MEM_HOST, t * 4, true, 0);
    Staged sout(ctx->be, out, where_out, rows * t * 32, false, 1);
    pc::gather_columns(ctx->be, (const uint32_t*)mat_dev, rows, n_cols, (const uint32_t*)sidx.dev, t, (uint32_t*)sout.dev);
    if (where_out == PC_MEM_HOST) ctx->be.copy_d2h(out, sout.dev, rows * t * 32); else ctx->be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_fr_lincomb(pc_ctx* ctx, pc_curve field_of, const void* const* polys, pc_mem where_in, const size_t* lens,
                      size_t k, const void* xi_host, void* out, pc_mem where_out, size_t n_out) {
  if (!pc_known_curve(field_of)) return PC_ERR_INVALID_ARG;
  return fr_lincomb_call(ctx, pc::field_ops(field_of), polys, where_in, lens, k, xi_host, out, where_out, n_out);
}

}  // extern "C"
