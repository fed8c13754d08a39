// C ABI of the gfx950 backend (include/pc_hip.h): G2 keys, the G2 MSM and MultilinearPC's setup, trim and open (multilinear_pc/mod.rs).
// This unit also instantiates everything templated on G2 (g2.hpp, fixed_base.hpp, MsmPlan<G2Of<C>, HipBackend>), BLS12-381 only,
// and nothing of G1: the G1 half of the setup goes through pc::curve_ops.
#include <chrono>
#include "abi.hpp"
#include "blocking_lane.hpp"
#include "fixed_base.hpp"

namespace pc {
namespace {

typedef G2Of<pc_curve_bls12_381> G2C;
typedef pc_curve_bls12_381::FrP FrP;
constexpr int G2_AW = AffD<G2C>::WORDS, G2_XW = XyzzD<G2C>::WORDS, FR_W = FrP::N;

// the key's one pipeline (table-free: the plan refuses a G2 table), created on first use
BlockingLane* g2_lane(pc_g2_srs* k) {
  if (k->lane) return k->lane;
  MsmConfig cfg = k->ctx->msm_cfg;
  cfg.tbl = nullptr; cfg.tbl_c = 0;
  cfg.K1 = 128;                  // a cooperative level's LDS tile: 128 points x 384 bytes = 48 KiB
  return k->lane = blocking_lane<G2C>(k->n, cfg, 0);
}

// the rounds of an opening with at most this many pairs run as one small kernel (k_small_msm) instead of the full pipeline
uint32_t small_round_max() {
  static const uint32_t v = []() { const char* e = getenv("PC_HIP_G2_SMALL_ROUND"); int x = e ? atoi(e) : 32; return (uint32_t)(x < 0 ? 0 : x > 128 ? 128 : x); }();
  return v;
}

// sum_j k_j P_j for n <= 128 pairs in ONE workgroup: every lane multiplies its pair (ScalarMulBody), a binary tree through LDS adds
// the products, lane 0 stores the XYZZ sum (the host normalises it: the tail).  blockDim = the power of two >= n, at least 64.
__global__ void __launch_bounds__(128) k_small_msm(ScalarMulBody<G2C> m, uint32_t n, uint32_t* out_xyzz) {
  typedef XyzzD<G2C> Pt;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  LdsPoints<G2C> lds{smem, blockDim.x};
  const uint32_t l = threadIdx.x;
  Pt v = l < n ? m.product(l) : Pt::infinity();
  for (uint32_t d = blockDim.x >> 1; d >= 1; d >>= 1) {
    lds.put(l, v);
    __syncthreads();
    if (l < d) v.add(lds.get(l + d));
    __syncthreads();
  }
  if (l == 0) v.store(out_xyzz);
}

void small_msm(HipBackend& be, const uint32_t* bases, const uint32_t* scalars_dev, uint32_t n, bool from_mont, uint32_t* out_host) {
  uint32_t* dres = (uint32_t*)be.workspace((size_t)G2_XW * 4);
  uint32_t block = 64; while (block < n) block <<= 1;
  ScalarMulBody<G2C> m{bases, scalars_dev, from_mont ? 1u : 0u};
  hipLaunchKernelGGL(k_small_msm, dim3(1), dim3(block), (size_t)block * G2_XW * 4, be.stream, m, n, dres);
  PC_HIP_CHECK(hipGetLastError());
  uint32_t xyzz[G2_XW];
  be.copy_d2h(xyzz, dres, sizeof(xyzz));
  host64::Xyzz64<G2C>::load(xyzz).store_affine(out_host);
}

}  // namespace
}  // namespace pc

using pc::G2C;
using pc::G2_AW;
using pc::FR_W;

static int g2_curve_check(pc_curve curve) {
  // BLS12-377's Fq2 is Fq[u] / (u^2 + 5) and fp2.hpp is written for u^2 + 1: no G2 of it here, and the id is refused like an unknown one
  if (!pc_known_curve(curve) || curve == PC_CURVE_BLS12_377) return PC_ERR_INVALID_ARG;
  return curve == PC_CURVE_BLS12_381 ? PC_OK : PC_ERR_UNSUPPORTED;
}

extern "C" {

int pc_hip_g2_srs_upload(pc_ctx* ctx, pc_curve curve, const void* bases, size_t n, size_t stride_bytes, pc_mem where, pc_g2_srs** out) {
  if (!ctx || !out || (!bases && n)) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(curve)) return rc;
  const size_t pb = (size_t)g2_point_bytes(curve);
  if (stride_bytes == 0) stride_bytes = pb;
  if (stride_bytes < pb) return PC_ERR_INVALID_ARG;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  if (where == PC_MEM_DEVICE && stride_bytes != pb) return PC_ERR_UNSUPPORTED;
  return key_make(ctx, out, [&]() { return g2_key_create(ctx, curve, n); }, g2_key_free, [&](pc_g2_srs* k) {
    key_base_fill(k, bases, n, stride_bytes, where);
    return (int)PC_OK;
  });
}

void pc_hip_g2_srs_free(pc_g2_srs* k) { key_free_locked(k, g2_key_free); }

size_t pc_hip_g2_srs_len(const pc_g2_srs* k) { return k ? k->n : 0; }

int pc_hip_g2_srs_bytes_resident(const pc_g2_srs* k, size_t out[4]) {
  if (!k || !out) return PC_ERR_INVALID_ARG;
  if (!k->ctx) { out[0] = out[1] = out[2] = out[3] = 0; return PC_OK; }
  std::lock_guard<std::recursive_mutex> lk(k->ctx->mu);
  g2_key_bytes(k, out);
  return PC_OK;
}

int pc_hip_g2_srs_read(pc_ctx* ctx, const pc_g2_srs* k, size_t offset, size_t count, void* out_host) { return key_base_read(ctx, k, offset, count, out_host); }

int pc_hip_g2_srs_pair_sums(pc_ctx* ctx, const pc_g2_srs* in, size_t off, size_t count, pc_g2_srs* out, size_t out_off) {
  if (!ctx || !in || !out || in->ctx != ctx || out->ctx != ctx || in->curve != out->curve) return PC_ERR_INVALID_ARG;
  if (off > in->n || count > (in->n - off) / 2 || out_off > out->n || count > out->n - out_off) return PC_ERR_INVALID_ARG;
  if (in == out && off < out_off + count && out_off < off + 2 * count) return PC_ERR_INVALID_ARG;      // overlapping ranges of one key
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    pc::pair_sums_run<G2C>(ctx->be, in->bases + off * (size_t)G2_AW, count, out->bases + out_off * (size_t)G2_AW);
    ctx->be.sync();
    return (int)PC_OK;
  });
}

void* pc_hip_g2_srs_device_ptr(const pc_g2_srs* k) { return k ? k->bases : nullptr; }

int pc_hip_ml_eq_evals(pc_ctx* ctx, pc_curve field_of, const void* t_host, unsigned nv, void* out_dev) {
  if (!ctx || !t_host || !out_dev || nv < 1) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(field_of)) return rc;
  if (nv > pc::ML_MAX_VARS) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    pc::MlEqBody<pc::FrP> b; b.out = (uint32_t*)out_dev; b.set_point((const uint32_t*)t_host, nv);
    ctx->be.launch(b, (size_t)1 << nv);
    ctx->be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_g2_fixed_base_batch_mul(pc_ctx* ctx, pc_curve curve, const void* h_host, const void* scalars_dev, size_t n, void* out_points_dev) {
  if (!ctx || !h_host || (n && (!scalars_dev || !out_points_dev))) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(curve)) return rc;
  if (n >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    pc::fixed_base_run<G2C>(ctx->be, (const uint32_t*)h_host, (const uint32_t*)scalars_dev, n, (uint32_t*)out_points_dev, pc::FIXED_BASE_K_ML);
    return (int)PC_OK;
  });
}

// points before level i of a key whose level 0 holds 2^nv points: 2^(nv+1) - 2^(nv-i+1)
static size_t ml_level_off(unsigned nv, unsigned i) { return ((size_t)2 << nv) - ((size_t)2 << (nv - i)); }

int pc_hip_ml_setup(pc_ctx* ctx, pc_curve curve, unsigned nv, const void* g_xy_host, const void* h_host, const void* t_host,
                    pc_srs** out_powers_of_g, pc_g2_srs** out_powers_of_h, void* g_mask_out_host) {
  if (!ctx || !g_xy_host || !h_host || !t_host || !out_powers_of_g || !out_powers_of_h || nv < 1) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(curve)) return rc;
  if (nv > 29) return PC_ERR_TOO_LARGE;      // a key holds fewer than 2^31 points
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  *out_powers_of_g = nullptr; *out_powers_of_h = nullptr;
  pc_srs* G = nullptr; pc_g2_srs* H = nullptr;
  const size_t n0 = (size_t)1 << nv;
  const pc::CurveOps& g1 = pc::curve_ops(curve);
  int rc = guarded(ctx, [&]() {
    G = key_create(ctx, curve, 2 * n0 - 2);
    if (!G) return (int)PC_ERR_OOM;
    H = g2_key_create(ctx, curve, 2 * n0 - 1);
    if (!H) return (int)PC_ERR_OOM;
    pc::HipBackend& be = ctx->be;
    // with timing on (pc_hip_set_timing) the four phases are bracketed on the host and left where pc_hip_last_msm_phases_ms reads
    // them: eq table, G1 level 0, G2 level 0, the upper levels
    const bool timed = be.timing;
    auto t_prev = std::chrono::steady_clock::now();
    int phase = 0;
    auto bracket = [&]() {
      if (!timed) return;
      be.sync();
      const auto now = std::chrono::steady_clock::now();
      ctx->phases[phase++] = std::chrono::duration<float, std::milli>(now - t_prev).count();
      t_prev = now;
    };
    if (timed) for (int i = 0; i < 8; i++) ctx->phases[i] = 0;
    // L_0[x] = prod_j e(t_j, bit_j(x)): the only level that is multiplied (mod.rs:36-62 multiplies all 2^(nv+1) - 2 scalars)
    CallBuf eq(be, 0, n0 * (size_t)FR_W * 4);
    pc::MlEqBody<pc::FrP> eb; eb.out = (uint32_t*)eq.dev; eb.set_point((const uint32_t*)t_host, nv);
    be.launch(eb, n0);
    bracket();
    g1.fixed_base(be, (const uint32_t*)g_xy_host, (const uint32_t*)eq.dev, n0, G->bases, pc::FIXED_BASE_K_ML);
    bracket();
    pc::fixed_base_run<G2C>(be, (const uint32_t*)h_host, (const uint32_t*)eq.dev, n0, H->bases, pc::FIXED_BASE_K_ML);
    bracket();
    // L_i[2b] + L_i[2b + 1] = L_{i+1}[b]: every higher level is the pair sums of the one below; the sum of the last one is 1
    for (unsigned i = 0; i + 1 < nv; i++) {
      const size_t off = ml_level_off(nv, i), m = n0 >> i;
      g1.pair_sums(be, G->bases + off * g1.aw, m / 2, G->bases + (off + m) * g1.aw);
      pc::pair_sums_run<G2C>(be, H->bases + off * G2_AW, m / 2, H->bases + (off + m) * G2_AW);
    }
    be.copy_h2d(H->bases + (2 * n0 - 2) * G2_AW, h_host, (size_t)G2_AW * 4);
    be.sync();
    bracket();
    if (g_mask_out_host)      // g_mask[i] = t_i * g (mod.rs:75): nv multiplications, on the host
      for (unsigned i = 0; i < nv; i++)
        g1.point_mul((const uint32_t*)g_xy_host, (const uint32_t*)t_host + (size_t)i * FR_W, (uint32_t*)g_mask_out_host + (size_t)i * g1.aw);
    return (int)PC_OK;
  });
  if (rc != PC_OK) { if (G) key_free(G); if (H) g2_key_free(H); return rc; }
  *out_powers_of_g = G; *out_powers_of_h = H;
  return PC_OK;
}

int pc_hip_ml_trim(pc_ctx* ctx, const pc_srs* powers_of_g, const pc_g2_srs* powers_of_h, unsigned nv, unsigned supported,
                   pc_srs** out_powers_of_g0, pc_g2_srs** out_pair_key) {
  if (!ctx || !powers_of_g || !powers_of_h || !out_powers_of_g0 || !out_pair_key) return PC_ERR_INVALID_ARG;
  if (powers_of_g->ctx != ctx || powers_of_h->ctx != ctx || nv < 1 || supported < 1 || supported > nv) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(powers_of_g->curve)) return rc;
  if (nv > 29) return PC_ERR_TOO_LARGE;
  if (powers_of_g->n != ((size_t)2 << nv) - 2 || powers_of_h->n != ((size_t)2 << nv) - 1) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  *out_powers_of_g0 = nullptr; *out_pair_key = nullptr;
  pc_srs* G = nullptr; pc_g2_srs* H = nullptr;
  const size_t n = (size_t)1 << supported;
  int rc = guarded(ctx, [&]() {
    G = key_create(ctx, powers_of_g->curve, n);
    if (!G) return (int)PC_ERR_OOM;
    H = g2_key_create(ctx, powers_of_h->curve, n - 1);
    if (!H) return (int)PC_ERR_OOM;
    // level nv - supported of G1; the pair sums of the G2 levels [nv - supported, nv) are the levels above them and h: the key's tail
    ctx->be.copy_d2d(G->bases, powers_of_g->bases + ml_level_off(nv, nv - supported) * (size_t)G->aw, n * (size_t)G->aw * 4);
    ctx->be.copy_d2d(H->bases, powers_of_h->bases + (powers_of_h->n - (n - 1)) * (size_t)G2_AW, (n - 1) * (size_t)G2_AW * 4);
    ctx->be.sync();
    return (int)PC_OK;
  });
  if (rc != PC_OK) { if (G) key_free(G); if (H) g2_key_free(H); return rc; }
  *out_powers_of_g0 = G; *out_pair_key = H;
  return PC_OK;
}

int pc_hip_g2_msm(pc_ctx* ctx, const pc_g2_srs* kc, size_t base_offset, const void* scalars, pc_scalar_form form, pc_mem where, size_t n,
                  void* out_xy, int* out_is_infinity) {
  pc_g2_srs* k = const_cast<pc_g2_srs*>(kc);
  if (!ctx || !k || !out_xy || k->ctx != ctx || base_offset > k->n) return PC_ERR_INVALID_ARG;
  const size_t avail = k->n - base_offset;      // msm_bigint semantics: min(bases.len(), scalars.len()) pairs
  if (n > avail) n = avail;
  if (n && !scalars) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    BlockingLane* L = pc::g2_lane(k);
    L->be.timing = ctx->be.timing;
    L->runner->run(k->bases, (uint32_t)base_offset, scalars, where, n, form == PC_SCALARS_MONTGOMERY, (uint32_t*)out_xy);
    if (n) lane_phases(ctx, L);      // (pc_hip_last_msm_shape, pc_hip_last_msm_phases_ms; an empty call plans nothing)
    if (out_is_infinity) *out_is_infinity = affine_is_zero((const uint32_t*)out_xy, G2_AW);
    return (int)PC_OK;
  });
}

int pc_hip_g2_points_sum(pc_curve curve, const void* points, size_t count, void* out_xy) {
  if (!out_xy || (count && !points)) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(curve)) return rc;
  pc::host64::points_sum<G2C>((const uint32_t*)points, count, (uint32_t*)out_xy);
  return PC_OK;
}

int pc_hip_g2_point_mul(pc_curve curve, const void* point, const void* scalar_mont, void* out_xy) {
  if (!point || !scalar_mont || !out_xy) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(curve)) return rc;
  pc::host64::scalar_mul<G2C>((const uint32_t*)point, pc::Fd<pc::FrP>::load((const uint32_t*)scalar_mont).from_mont().l, (uint32_t*)out_xy);
  return PC_OK;
}

int pc_hip_ml_fold(pc_ctx* ctx, pc_curve field_of, const void* r_in_dev, size_t n_half, const void* z_host, void* r_out_dev, void* q_dev) {
  if (!ctx || !z_host || (n_half && (!r_in_dev || !r_out_dev || !q_dev))) return PC_ERR_INVALID_ARG;
  if (int rc = g2_curve_check(field_of)) return rc;
  if (n_half >= (1ull << 31)) return PC_ERR_TOO_LARGE;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    if (!n_half) return (int)PC_OK;
    pc::MlFoldBody<pc::FrP> b; b.r_in = (const uint32_t*)r_in_dev; b.r_out = (uint32_t*)r_out_dev; b.q = (uint32_t*)q_dev;
    memcpy(b.z, z_host, sizeof(b.z));
    ctx->be.launch(b, n_half);
    ctx->be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_ml_open(pc_ctx* ctx, const pc_g2_srs* kc, const void* evals, pc_mem where, unsigned nv, const void* point_host, void* proofs_out,
                   int* out_is_infinity) {
  pc_g2_srs* k = const_cast<pc_g2_srs*>(kc);
  if (!ctx || !k || k->ctx != ctx || !evals || !point_host || !proofs_out || nv < 1 || nv > 30) return PC_ERR_INVALID_ARG;
  const size_t n = (size_t)1 << nv;
  if (k->n != n - 1) return PC_ERR_INVALID_ARG;      // the pair sums of powers_of_h[0 .. nv)
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const size_t fb = (size_t)FR_W * 4;
    // r ping-pong (n/2 and n/4 elements; round 0 reads the evaluations where they are, or their staged copy) and q (n/2)
    Staged ev(ctx->be, evals, where, n * fb, true, 0);
    CallBuf work(ctx->be, 1, (n / 2 + n / 2 + (n / 4 ? n / 4 : 1)) * fb);
    uint32_t* q = (uint32_t*)work.dev;
    uint32_t* rbuf[2] = {q + (n / 2) * FR_W, q + (n / 2 + n / 2) * FR_W};
    const uint32_t* r_in = (const uint32_t*)ev.dev;
    BlockingLane* L = pc::g2_lane(k);
    L->be.timing = false;
    for (unsigned i = 0; i < nv; i++) {
      const size_t half = n >> (i + 1), off = n - (n >> i);
      uint32_t* r_out = rbuf[i & 1];
      pc::MlFoldBody<pc::FrP> b; b.r_in = r_in; b.r_out = r_out; b.q = q;
      memcpy(b.z, (const uint8_t*)point_host + (size_t)i * fb, sizeof(b.z));
      ctx->be.launch(b, half);
      ctx->be.sync();      // the MSM runs on the key's own queue
      uint32_t* proof = (uint32_t*)proofs_out + (size_t)i * G2_AW;
      if (half <= pc::small_round_max()) pc::small_msm(ctx->be, k->bases + off * (size_t)G2_AW, q, (uint32_t)half, true, proof);
      else L->runner->run(k->bases, (uint32_t)off, q, PC_MEM_DEVICE, half, true, proof);
      if (out_is_infinity) out_is_infinity[i] = affine_is_zero(proof, G2_AW);
      r_in = r_out;
    }
    return (int)PC_OK;
  });
}

}  // extern "C"
