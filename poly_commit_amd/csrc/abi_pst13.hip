// C ABI of the gfx950 backend (include/pc_hip.h): MarlinPST13 -- the dense lexicographic layout of a multivariate key and
// polynomial, the monomial evaluations of setup, scatter, the division along every variable, commit and open against one resident
// key, the re-ranking of trim.  The kernels are csrc/pst13.hpp (the field-dependent ones through FieldOps); the MSMs and the key are
// the existing entry points' (pc_hip_msm, pc_hip_msm_batch), called under the context's recursive lock.
#include <string.h>
#include "abi.hpp"
#include "pst13.hpp"

namespace {

constexpr size_t EB = 32;                      // bytes of one Fr
constexpr size_t MAXV = PC_HIP_PST13_MAX_VARS;
static_assert(PC_HIP_PST13_MAX_VARS == pc::PST13_MAX_VARS && PC_HIP_PST13_MAX_DEGREE == pc::PST13_MAX_DEGREE, "pc_hip.h and pst13.hpp name the same limits");

// C(v + r, v), or 0 from 2^28 on
size_t monomials(size_t v, size_t r) {
  const size_t lo = std::min(v, r), hi = std::max(v, r);
  uint64_t c = 1;
  for (size_t i = 1; i <= lo; i++) {
    c = c * (hi + i) / i;                                              // exact: c is C(hi + i - 1, i - 1) before
    if (c >> pc::PST13_LOG2_MAX_LEN) return 0;
  }
  return (size_t)c;
}

int shape_status(size_t n, size_t d) {
  if (!n || !d) return PC_ERR_INVALID_ARG;
  if (n > MAXV || (n >= 2 && d > PC_HIP_PST13_MAX_DEGREE) || d >= (1ull << pc::PST13_LOG2_MAX_LEN) || !monomials(n, d)) return PC_ERR_TOO_LARGE;
  return PC_OK;
}

// the layout (n, d) of a call whose shape_status is PC_OK
struct Layout {
  uint32_t n, d; size_t M;
  std::vector<uint32_t> T;                     // pst13_table(n, d); empty for a univariate polynomial of degree above 255 (no kernel reads it)
  std::vector<size_t> pre;                     // pre[i] = N(n - i, d): slots of a polynomial in X_i .. X_{n-1}, i <= n
  std::vector<uint64_t> off; size_t qtotal = 0;      // quotient i at off[i] of the packed quotients, pre[i] slots
  Layout(size_t n_, size_t d_) : n((uint32_t)n_), d((uint32_t)d_), M(monomials(n_, d_)), pre(n_ + 1), off(n_) {
    if (d <= PC_HIP_PST13_MAX_DEGREE) T = pc::pst13_table(n, d);
    for (uint32_t i = 0; i <= n; i++) pre[i] = monomials(n - i, d);
    for (uint32_t i = 0; i < n; i++) { off[i] = qtotal; qtotal += pre[i]; }
  }
  uint32_t words() const { return (uint32_t)T.size(); }
};

size_t al(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct Arena {
  char* p;
  void* take(size_t bytes) { void* r = p; p += al(bytes); return r; }
};

bool key_too_short(const pc_ctx* ctx, const pc_srs* srs, size_t base_offset, size_t need) {
  return srs->ctx != ctx || base_offset > srs->n || need > srs->n - base_offset;
}

const uint32_t* table_to(pc::HipBackend& be, Arena& a, const Layout& L) {
  uint32_t* t = (uint32_t*)a.take((size_t)L.words() * 4);
  if (L.words()) be.copy_h2d(t, L.T.data(), (size_t)L.words() * 4);
  return t;
}

// terms -> the dense vector `out` (M slots, device).  exps / coeffs: device, or host (copied into the arena)
size_t scatter_bytes(const Layout& L, size_t terms, pc_mem where) {
  return al(32) + al(L.M * 4) + (where == PC_MEM_HOST ? al(terms * L.n) + al(terms * EB) : 0);
}
int scatter_dev(pc_ctx* ctx, pc_curve field_of, const Layout& L, const uint32_t* table, Arena& a, const void* exps, const void* coeffs, pc_mem where,
                size_t terms, uint32_t* out) {
  pc::HipBackend& be = ctx->be;
  uint32_t* flags = (uint32_t*)a.take(32);
  uint32_t* owner = (uint32_t*)a.take(L.M * 4);
  be.memset(out, 0, L.M * EB);
  if (!terms) return PC_OK;
  if (where == PC_MEM_HOST) {
    void* e = a.take(terms * L.n); void* c = a.take(terms * EB);
    be.copy_h2d(e, exps, terms * L.n); be.copy_h2d(c, coeffs, terms * EB);
    exps = e; coeffs = c;
  }
  be.memset(flags, 0, 32);
  be.memset(owner, 0, L.M * 4);
  pc::Pst13ClaimBody claim{(const uint8_t*)exps, owner, flags, L.n, L.d};
  pc::pst13_launch(be, claim, terms, table, L.words());
  pc::field_ops(field_of).pst13_write(be, table, L.n, L.d, (const uint8_t*)exps, (const uint32_t*)coeffs, terms, owner, flags, out);
  uint32_t f = 0;
  be.copy_d2h(&f, flags, 4);
  if (f) { ctx->last_error = (f & pc::PST13_FLAG_DEGREE) ? "pst13: a term of degree above the layout's" : "pst13: a repeated exponent tuple"; return PC_ERR_INVALID_ARG; }
  return PC_OK;
}

// the division of p (M slots, device, untouched) at z: quotient i at quot + off[i]; *value = p(z)
size_t divide_bytes(const Layout& L) { return L.n == 1 ? al(L.M * EB) : 2 * al(L.pre[1] * EB); }
void divide_dev(pc_ctx* ctx, pc_curve field_of, const Layout& L, const uint32_t* table, Arena& a, const uint32_t* p, const uint32_t* z_host,
                uint32_t* quot, void* value_host) {
  pc::HipBackend& be = ctx->be;
  const pc::FieldOps& F = pc::field_ops(field_of);
  if (L.n == 1) {                              // natural order: the division scan (out[0] = p(z), out[1 ..] = the witness polynomial)
    uint32_t* tmp = (uint32_t*)a.take(L.M * EB);
    F.div_scan(be, p, L.M, z_host, nullptr, tmp, scan_fan());
    be.copy_d2d(quot, tmp + 8, (L.M - 1) * EB);
    be.memset(quot + (L.M - 1) * 8, 0, EB);
    be.copy_d2h(value_host, tmp, EB);
    return;
  }
  uint32_t* ping = (uint32_t*)a.take(L.pre[1] * EB); uint32_t* pong = (uint32_t*)a.take(L.pre[1] * EB);
  const uint32_t* last = F.pst13_divide(be, table, L.T.data(), L.n, L.d, p, z_host, quot, L.off.data(), ping, pong);
  be.copy_d2h(value_host, last, EB);
}

int terms_status(const Layout& L, const void* exps, const void* coeffs, size_t terms) {
  if (terms && (!exps || !coeffs)) return PC_ERR_INVALID_ARG;
  if (terms >= 0xFFFFFFFFull || L.d > PC_HIP_PST13_MAX_DEGREE) return PC_ERR_TOO_LARGE;      // an exponent is one byte
  return PC_OK;
}

}  // namespace

extern "C" {

size_t pc_hip_pst13_key_len(size_t num_vars, size_t degree) {
  return shape_status(num_vars, degree) == PC_OK ? monomials(num_vars, degree) : 0;
}

int pc_hip_pst13_rank(size_t num_vars, size_t degree, const uint8_t* exps, size_t count, uint32_t* out_ranks) {
  if ((count && (!exps || !out_ranks))) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  if (degree > PC_HIP_PST13_MAX_DEGREE) return PC_ERR_TOO_LARGE;
  const Layout L(num_vars, degree);
  for (size_t t = 0; t < count; t++) {
    pc::Pst13Exps e;
    if (pc::pst13_load_exps(exps + t * L.n, L.n, e) > L.d) return PC_ERR_INVALID_ARG;
    out_ranks[t] = pc::pst13_rank(L.T.data(), L.d + 1, e, 0, L.n, L.d);
  }
  return PC_OK;
}

int pc_hip_pst13_unrank(size_t num_vars, size_t degree, const uint32_t* ranks, size_t count, uint8_t* out_exps) {
  if ((count && (!ranks || !out_exps))) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  if (degree > PC_HIP_PST13_MAX_DEGREE) return PC_ERR_TOO_LARGE;
  const Layout L(num_vars, degree);
  for (size_t t = 0; t < count; t++) {
    if (ranks[t] >= L.M) return PC_ERR_INVALID_ARG;
    pc::Pst13Exps e; e.clear();
    pc::pst13_unrank(L.T.data(), L.d + 1, ranks[t], 0, L.n, L.d, e);
    for (uint32_t j = 0; j < L.n; j++) out_exps[t * L.n + j] = (uint8_t)e.get(j);
  }
  return PC_OK;
}

int pc_hip_pst13_monomial_evals(pc_ctx* ctx, pc_curve field_of, size_t num_vars, size_t degree, const void* betas_host, void* out_dev) {
  if (!ctx || !pc_known_curve(field_of) || !betas_host || !out_dev) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    const Layout L(num_vars, degree);
    const pc::FieldOps& F = pc::field_ops(field_of);
    if (L.n == 1) { F.fr_powers(ctx->be, (const uint32_t*)betas_host, L.M, (uint32_t*)out_dev); return (int)PC_OK; }
    const pc::CurveOps& C = pc::curve_ops(field_of);
    const size_t row = (size_t)L.d + 1;
    std::vector<uint32_t> pw((size_t)L.n * row * 8);                   // pw[j][t] = beta_j^t
    for (uint32_t j = 0; j < L.n; j++) {
      C.fr_one(&pw[j * row * 8]);
      for (size_t t = 1; t < row; t++) C.fr_mul(&pw[(j * row + t - 1) * 8], (const uint32_t*)betas_host + (size_t)j * 8, &pw[(j * row + t) * 8]);
    }
    CallBuf buf(ctx->be, 1, al((size_t)L.words() * 4) + al(pw.size() * 4));
    Arena a{(char*)buf.dev};
    const uint32_t* table = table_to(ctx->be, a, L);
    uint32_t* pwd = (uint32_t*)a.take(pw.size() * 4);
    ctx->be.copy_h2d(pwd, pw.data(), pw.size() * 4);
    F.pst13_monomials(ctx->be, table, L.n, L.d, L.M, pwd, (uint32_t*)out_dev);
    ctx->be.sync();
    return (int)PC_OK;
  });
}

int pc_hip_pst13_scatter(pc_ctx* ctx, pc_curve field_of, size_t num_vars, size_t degree, const void* exps, const void* coeffs, pc_mem where,
                         size_t n_terms, void* out_dev) {
  if (!ctx || !pc_known_curve(field_of) || !out_dev) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  const Layout L(num_vars, degree);
  if ((rc = terms_status(L, exps, coeffs, n_terms)) != PC_OK) return rc;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    CallBuf buf(ctx->be, 1, al((size_t)L.words() * 4) + scatter_bytes(L, n_terms, where));
    Arena a{(char*)buf.dev};
    const uint32_t* table = table_to(ctx->be, a, L);
    const int r = scatter_dev(ctx, field_of, L, table, a, exps, coeffs, where, n_terms, (uint32_t*)out_dev);
    ctx->be.sync();
    return r;
  });
}

int pc_hip_pst13_divide(pc_ctx* ctx, pc_curve field_of, size_t num_vars, size_t degree, const void* poly, pc_mem where, const void* point_host,
                        void* quotients_dev, size_t capacity_elems, size_t* offsets_host, void* value_host) {
  if (!ctx || !pc_known_curve(field_of) || !poly || !point_host || !quotients_dev || !offsets_host || !value_host) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  const Layout L(num_vars, degree);
  if (capacity_elems < L.qtotal) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sin(ctx->be, poly, where, L.M * EB, true, 0);
    CallBuf buf(ctx->be, 1, al((size_t)L.words() * 4) + divide_bytes(L));
    Arena a{(char*)buf.dev};
    const uint32_t* table = table_to(ctx->be, a, L);
    divide_dev(ctx, field_of, L, table, a, (const uint32_t*)sin.dev, (const uint32_t*)point_host, (uint32_t*)quotients_dev, value_host);
    for (uint32_t i = 0; i < L.n; i++) offsets_host[i] = (size_t)L.off[i];
    return (int)PC_OK;
  });
}

int pc_hip_pst13_commit(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, size_t num_vars, size_t degree, const void* dense, pc_mem where_dense,
                        const void* exps, const void* coeffs, pc_mem where_terms, size_t n_terms, void* out_xy, int* out_is_infinity) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !out_xy || (dense && (exps || coeffs || n_terms))) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  const Layout L(num_vars, degree);
  if (!dense && (rc = terms_status(L, exps, coeffs, n_terms)) != PC_OK) return rc;
  if (key_too_short(ctx, srs, base_offset, L.M)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (dense) return pc_hip_msm(ctx, srs, base_offset, dense, PC_SCALARS_MONTGOMERY, where_dense, L.M, out_xy, out_is_infinity);
  return guarded(ctx, [&]() {
    CallBuf buf(ctx->be, 1, al((size_t)L.words() * 4) + al(L.M * EB) + scatter_bytes(L, n_terms, where_terms));
    Arena a{(char*)buf.dev};
    const uint32_t* table = table_to(ctx->be, a, L);
    uint32_t* p = (uint32_t*)a.take(L.M * EB);
    const int r = scatter_dev(ctx, srs->curve, L, table, a, exps, coeffs, where_terms, n_terms, p);
    if (r != PC_OK) return r;
    ctx->be.sync();
    return pc_hip_msm(ctx, srs, base_offset, p, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, L.M, out_xy, out_is_infinity);
  });
}

int pc_hip_pst13_open(pc_ctx* ctx, const pc_srs* srs_c, size_t base_offset, size_t num_vars, size_t degree, const void* dense, pc_mem where_dense,
                      const void* exps, const void* coeffs, pc_mem where_terms, size_t n_terms, const void* point_host, void* out_xy,
                      int* out_is_infinity, void* value_host) {
  pc_srs* srs = const_cast<pc_srs*>(srs_c);
  if (!ctx || !srs || !point_host || !out_xy || !value_host || (dense && (exps || coeffs || n_terms))) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  const Layout L(num_vars, degree);
  if (!dense && (rc = terms_status(L, exps, coeffs, n_terms)) != PC_OK) return rc;
  if (key_too_short(ctx, srs, base_offset, L.M)) return PC_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  return guarded(ctx, [&]() {
    Staged sin(ctx->be, dense, dense ? where_dense : PC_MEM_DEVICE, L.M * EB, true, 0);
    // arena: the table | the polynomial (from terms) | the n quotients | the division's dividends | the scatter's words
    CallBuf buf(ctx->be, 1, al((size_t)L.words() * 4) + (dense ? 0 : al(L.M * EB) + scatter_bytes(L, n_terms, where_terms)) + al(L.qtotal * EB) + divide_bytes(L));
    Arena a{(char*)buf.dev};
    const uint32_t* table = table_to(ctx->be, a, L);
    const uint32_t* p = (const uint32_t*)sin.dev;
    if (!dense) {
      uint32_t* pt = (uint32_t*)a.take(L.M * EB);
      const int r = scatter_dev(ctx, srs->curve, L, table, a, exps, coeffs, where_terms, n_terms, pt);
      if (r != PC_OK) return r;
      p = pt;
    }
    uint32_t* quot = (uint32_t*)a.take(L.qtotal * EB);
    divide_dev(ctx, srs->curve, L, table, a, p, (const uint32_t*)point_host, quot, value_host);      // drains the queue (p(z) comes back)
    // MSM i over the prefix [base_offset, base_offset + N(n - i, d)): w_i has no variable before X_i (mod.rs:457-469 without a gather);
    // a univariate quotient has d coefficients
    std::vector<const void*> ptrs(L.n); std::vector<size_t> lens(L.n), offs(L.n, base_offset);
    memset(ctx->pst13_shape, 0, sizeof(ctx->pst13_shape));
    ctx->pst13_shape[0] = L.n; ctx->pst13_shape[1] = L.n == 1;
    for (uint32_t i = 0; i < L.n; i++) {
      ptrs[i] = quot + (size_t)L.off[i] * 8; lens[i] = L.n == 1 ? L.M - 1 : L.pre[i];
      ctx->pst13_shape[2 + i] = (uint32_t)lens[i];
    }
    return pc_hip_msm_batch(ctx, srs, offs.data(), ptrs.data(), lens.data(), L.n, PC_SCALARS_MONTGOMERY, PC_MEM_DEVICE, out_xy, out_is_infinity);
  });
}

int pc_hip_pst13_trim(pc_ctx* ctx, const pc_srs* srs, size_t base_offset, size_t num_vars, size_t degree, size_t supported_degree, pc_srs** out) {
  if (out) *out = nullptr;
  if (!ctx || !srs || !out || !supported_degree || supported_degree > degree) return PC_ERR_INVALID_ARG;
  int rc = shape_status(num_vars, degree);
  if (rc != PC_OK) return rc;
  const Layout L(num_vars, degree);
  if (key_too_short(ctx, srs, base_offset, L.M)) return PC_ERR_INVALID_ARG;
  const size_t Ms = monomials(num_vars, supported_degree);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  pc_srs* k = nullptr;
  rc = guarded(ctx, [&]() {
    k = key_create(ctx, srs->curve, Ms);
    if (!k) return (int)PC_ERR_OOM;
    const uint32_t* in = srs->bases + base_offset * (size_t)srs->aw;
    if (L.n == 1) { ctx->be.copy_d2d(k->bases, in, Ms * (size_t)srs->aw * 4); ctx->be.sync(); return (int)PC_OK; }
    CallBuf buf(ctx->be, 1, al((size_t)L.words() * 4));
    Arena a{(char*)buf.dev};
    const uint32_t* table = table_to(ctx->be, a, L);
    pc::Pst13RerankBody b{in, k->bases, L.n, L.d, (uint32_t)supported_degree, (uint32_t)srs->aw};
    pc::pst13_launch(ctx->be, b, Ms, table, L.words());
    ctx->be.sync();
    return (int)PC_OK;
  });
  if (rc != PC_OK) { if (k) (void)guarded(ctx, [&]() { key_free(k); return (int)PC_OK; }); return rc; }
  *out = k;
  return PC_OK;
}

int pc_hip_last_pst13_shape(const pc_ctx* ctx, uint32_t out[34]) {
  static_assert(sizeof(ctx->pst13_shape) == 34 * 4 && 34 == 2 + PC_HIP_PST13_MAX_VARS, "pc_hip.h sizes the caller's array");
  if (!ctx || !out) return PC_ERR_INVALID_ARG;
  memcpy(out, ctx->pst13_shape, sizeof(ctx->pst13_shape));
  return PC_OK;
}

}  // extern "C"
