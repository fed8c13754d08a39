// C++ host mirror of the Brakedown linear code, above the C ABI.
//
//   ent / ceil_mul                              poly-commit/src/utils.rs:26-39
//   SprsMat {new_from_flat, new_from_columns, row_mul}   linear_codes/utils.rs:20-107
//   BrakedownPCParams {default, new, mat_size, cn, dn, codeword_len, make_mat}   linear_codes/brakedown.rs:103-340
//   MultilinearBrakedown {encode, tensor}       linear_codes/multilinear_brakedown/mod.rs:56-122
//   BrakedownPCS {commit, open, check}          LinearCodePCS over this code: linear_codes/mod.rs:228-503 (no hiding: the reference has none)
// The matrices come from the CALLER's generator (make_mat draws from it in the reference's order); encode runs on the device through
// pc_hip_brakedown_encode, encode_host is the reference's loop on the host (the CPU baseline of tools/brakedown_timing.py and the
// cross-check of the device path).
#pragma once
#include <math.h>
#include <thread>
#include <tuple>
#include "linear_codes.hpp"

namespace pc_host {

typedef std::tuple<size_t, size_t, size_t> Dim;      // (n rows, m columns, d non-zeros per row)
typedef std::pair<size_t, size_t> Ratio;

inline double ent(double x) { return (x == 0.0 || x == 1.0) ? 0.0 : -x * log2(x) - (1.0 - x) * log2(1.0 - x); }
inline size_t ceil_mul(size_t a, Ratio b) { return (a * b.first + b.second - 1) / b.second; }
inline double ratio(Ratio a) { return (double)a.first / (double)a.second; }

// CSC (utils.rs:20-37)
template <class E>
struct SprsMat {
  typedef FrT<E> Fr;
  size_t n = 0, m = 0, d = 0;
  std::vector<size_t> ind_ptr; std::vector<size_t> col_ind; std::vector<Fr> val;
  // v.M (utils.rs:41-52)
  std::vector<Fr> row_mul(const Fr* v) const {
    std::vector<Fr> out(m);
    for (size_t j = 0; j < m; j++) {
      Fr acc = Fr::zero();
      for (size_t k = ind_ptr[j]; k < ind_ptr[j + 1]; k++) acc = acc + v[col_ind[k]] * val[k];
      out[j] = acc;
    }
    return out;
  }
  // column-major dense list of m * n elements (utils.rs:56-81)
  static SprsMat new_from_flat(size_t n, size_t m, size_t d, const std::vector<Fr>& list) {
    SprsMat s; s.n = n; s.m = m; s.d = d; s.ind_ptr.assign(m + 1, 0);
    for (size_t i = 0; i < m; i++) {
      for (size_t c = 0; c < n; c++) if (!list[i * n + c].is_zero()) { s.ind_ptr[i + 1]++; s.col_ind.push_back(c); s.val.push_back(list[i * n + c]); }
      s.ind_ptr[i + 1] += s.ind_ptr[i];
    }
    return s;
  }
  // per column, its (row, value) entries (utils.rs:82-106)
  static SprsMat new_from_columns(size_t n, size_t m, size_t d, const std::vector<std::vector<std::pair<size_t, Fr>>>& list) {
    SprsMat s; s.n = n; s.m = m; s.d = d; s.ind_ptr.assign(m + 1, 0);
    for (size_t j = 0; j < m; j++) {
      for (auto& e : list[j]) { s.col_ind.push_back(e.first); s.val.push_back(e.second); }
      s.ind_ptr[j + 1] = s.ind_ptr[j] + list[j].size();
    }
    return s;
  }
};

template <class E>
struct BrakedownPCParams {
  typedef FrT<E> Fr;
  size_t sec_param = 128; Ratio alpha{178, 1000}, beta{61, 1000}, rho_inv{1521, 1000}; size_t base_len = 30;      // brakedown.rs:111-115
  size_t n = 0, m = 0, m_ext = 0;
  std::vector<Dim> a_dims, b_dims; std::vector<size_t> start, end;
  std::vector<SprsMat<E>> a_mats, b_mats;
  bool check_well_formedness = true;
  struct Constants { Ratio a, b, r; std::pair<double, double> c, d; };

  static std::pair<double, double> cn_const(Ratio a_, Ratio b_) {
    const double a = ratio(a_), b = ratio(b_), arg = 1.28 * b / a;
    return {ent(b) + a * ent(arg), -b * log2(arg)};
  }
  static std::pair<double, double> dn_const(Ratio a_, Ratio b_, Ratio r_) {
    const double mu = (double)(r_.first * (a_.second - a_.first) - r_.second * a_.second) / (double)(r_.second * a_.second);
    const double nu = (double)(b_.first * (a_.second + a_.first) * 100 + 3 * b_.second * a_.second) / (double)(b_.second * a_.second * 100);
    const double a = ratio(a_), b = ratio(b_), r = ratio(r_), nm = nu / mu;
    return {r * a * ent(b / r) + mu * ent(nm), -a * b * log2(nm)};
  }
  static size_t cn(size_t n, const Constants& ct) {
    const size_t lo = std::max(ceil_mul(n, {32 * ct.b.first, 25 * ct.b.second}), 4 + ceil_mul(n, ct.b));
    return std::min(lo, (size_t)ceil((110.0 / (double)n + ct.c.first) / ct.c.second));
  }
  static size_t dn(size_t n, const Constants& ct, unsigned modulus_bits) {
    const size_t lo = ceil_mul(n, {2 * ct.b.first, ct.b.second}) + (size_t)ceil((double)(ceil_mul(n, ct.r) - n + 110) / (double)modulus_bits);
    return std::min(lo, (size_t)ceil((110.0 / (double)n + ct.d.first) / ct.d.second));
  }
  // brakedown.rs:260-288
  static void mat_size(size_t n, size_t base_len, const Constants& ct, unsigned modulus_bits, std::vector<Dim>& a_dims, std::vector<Dim>& b_dims) {
    a_dims.clear(); b_dims.clear();
    while (n >= base_len) {
      const size_t m = ceil_mul(n, ct.a);
      a_dims.push_back(Dim(n, m, std::min(cn(n, ct), m)));      // can't generate more nonzero entries than there are columns
      n = m;
    }
    for (auto& ad : a_dims) {
      const size_t bn = ceil_mul(std::get<1>(ad), ct.r), bm = ceil_mul(std::get<0>(ad), ct.r) - std::get<0>(ad) - bn;
      b_dims.push_back(Dim(bn, bm, std::min(dn(bn, ct, modulus_bits), bm)));
    }
  }
  static size_t codeword_len(const std::vector<Dim>& a_dims, const std::vector<Dim>& b_dims) {      // brakedown.rs:292-299
    size_t s = std::get<0>(b_dims.back());
    for (auto& d : b_dims) s += std::get<1>(d);
    for (auto& d : a_dims) s += std::get<0>(d);
    return s;
  }
  // make_mat (brakedown.rs:305-333) over the caller's generator: gen.next_u64() and gen.template nonzero<E>(), drawn in the reference's
  // order -- the d column indices of a row (Fisher-Yates on a list that is not reset between rows), then its d values
  template <class Gen>
  static SprsMat<E> make_mat(size_t n, size_t m, size_t d, Gen& gen) {
    std::vector<size_t> tmp(m); for (size_t i = 0; i < m; i++) tmp[i] = i;
    std::vector<std::vector<std::pair<size_t, Fr>>> mat(m);
    std::vector<size_t> idxs(d);
    for (size_t i = 0; i < n; i++) {
      for (size_t j = 0; j < d; j++) { const size_t r = (size_t)(gen.next_u64() % (uint64_t)(m - j)); std::swap(tmp[r], tmp[m - 1 - j]); idxs[j] = tmp[m - 1 - j]; }
      for (size_t j : idxs) mat[j].push_back({i, gen.template nonzero<E>()});
    }
    return SprsMat<E>::new_from_columns(n, m, d, mat);
  }
  // the shape of `default` (brakedown.rs:116-122): n, m, a_dims, b_dims, m_ext, start, end -- no matrices yet; false: InvalidParameters
  bool default_shape(size_t poly_len, unsigned modulus_bits = E::C::FrP::BITS) {
    const long t = calculate_t((int)modulus_bits, sec_param, beta.first * rho_inv.second, beta.second * rho_inv.first, poly_len);
    if (t <= 0) return false;
    n = (size_t)1 << ark_log2((size_t)ceil(sqrt((double)ceil_div(2 * poly_len, (size_t)t))));
    m = ceil_div(poly_len, n);
    const Constants ct{alpha, beta, rho_inv, cn_const(alpha, beta), dn_const(alpha, beta, rho_inv)};
    mat_size(m, base_len, ct, modulus_bits, a_dims, b_dims);
    finish();
    return true;
  }
  // BrakedownPCParams::default: the shape, then make_all(a_dims), make_all(b_dims) from the same generator (brakedown.rs:123-124)
  template <class Gen>
  bool make_default(size_t poly_len, Gen& gen) {
    if (!default_shape(poly_len)) return false;
    a_mats.clear(); b_mats.clear();
    for (auto& d : a_dims) a_mats.push_back(make_mat(std::get<0>(d), std::get<1>(d), std::get<2>(d), gen));
    for (auto& d : b_dims) b_mats.push_back(make_mat(std::get<0>(d), std::get<1>(d), std::get<2>(d), gen));
    return true;
  }
  // BrakedownPCParams::new (brakedown.rs:163-181): m_ext, start, end from the dimensions
  void finish() {
    m_ext = a_dims.empty() ? ceil_mul(m, rho_inv) : codeword_len(a_dims, b_dims);
    start.clear(); end.clear();
    size_t acc = 0; for (auto& d : a_dims) { acc += std::get<0>(d); start.push_back(acc); }
    acc = m_ext; for (auto& d : b_dims) { acc -= std::get<1>(d); end.push_back(acc); }
  }
  std::pair<size_t, size_t> distance() const { return {rho_inv.second * beta.first, rho_inv.first * beta.second}; }
  std::pair<size_t, size_t> compute_dimensions(size_t) const { return {n, m}; }
  long num_queries() const { auto d = distance(); return calculate_t(E::C::FrP::BITS, sec_param, d.first, d.second, m_ext); }

  // the resident copy of the matrices (pc_hip_brakedown_code_create); the caller frees it with pc_hip_brakedown_code_free
  Error upload(pc_ctx* ctx, pc_lincode** code) const {
    std::vector<size_t> dims, ind_ptr; std::vector<uint32_t> col_ind; std::vector<Fr> val;
    for (const std::vector<SprsMat<E>>* ms : {&a_mats, &b_mats})
      for (const SprsMat<E>& s : *ms) {
        dims.push_back(s.n); dims.push_back(s.m); dims.push_back(s.d);
        ind_ptr.insert(ind_ptr.end(), s.ind_ptr.begin(), s.ind_ptr.end());
        for (size_t c : s.col_ind) col_ind.push_back((uint32_t)c);
        val.insert(val.end(), s.val.begin(), s.val.end());
      }
    const int rc = pc_hip_brakedown_code_create(ctx, E::ID, m, m_ext, a_mats.size(), dims.data(), ind_ptr.data(), col_ind.data(), val.data(), val.size(), code);
    if (rc != PC_OK) { Error e; e.kind = rc == PC_ERR_INVALID_ARG ? Error::InvalidParameters : Error::Backend; e.msg = pc_hip_strerror(rc); return e; }
    return Error();
  }
};

template <class E>
struct MultilinearBrakedown {
  typedef FrT<E> Fr;
  // naive_reed_solomon (mod.rs:111-122)
  static void naive_reed_solomon(std::vector<Fr>& cw, size_t s, size_t ie, size_t oe) {
    std::vector<Fr> res(oe - s, Fr::zero());
    Fr x = Fr::one();
    for (Fr& r : res) {
      for (size_t j = ie; j-- > s;) r = r * x + cw[j];
      x = x + Fr::one();
    }
    for (size_t i = 0; i < res.size(); i++) cw[s + i] = res[i];
  }
  // encode (mod.rs:56-84) on the host, the last loop as written there: level 0 FIRST (no `.rev()`), so it reads zeros where the
  // later levels write
  static Error encode_host(const Fr* msg, size_t len, const BrakedownPCParams<E>& pp, std::vector<Fr>& cw) {
    if (len != pp.m) { Error e; e.kind = Error::IncorrectInputLength; e.msg = "EncodingError"; return e; }
    cw.assign(msg, msg + len);
    for (size_t i = 0; i < pp.start.size(); i++) {
      std::vector<Fr> src = pp.a_mats[i].row_mul(cw.data() + pp.start[i] - std::get<0>(pp.a_dims[i]));
      cw.insert(cw.end(), src.begin(), src.end());
    }
    cw.resize(pp.m_ext, Fr::zero());
    const size_t rss = pp.start.empty() ? 0 : pp.start.back();
    const size_t rsie = rss + (pp.a_dims.empty() ? pp.m : std::get<1>(pp.a_dims.back()));
    const size_t rsoe = pp.end.empty() ? pp.m_ext : pp.end.back();
    naive_reed_solomon(cw, rss, rsie, rsoe);
    for (size_t i = 0; i < pp.start.size(); i++) {
      std::vector<Fr> src = pp.b_mats[i].row_mul(cw.data() + pp.start[i]);
      for (size_t k = 0; k < src.size(); k++) cw[pp.end[i] + k] = src[k];
    }
    return Error();
  }
  // every row of a matrix on `threads` host threads (rows are independent, linear_codes/mod.rs:131-135)
  static void encode_rows_host(const Matrix<E>& mat, const BrakedownPCParams<E>& pp, Matrix<E>& ext, unsigned threads) {
    ext.n = mat.n; ext.m = pp.m_ext; ext.entries.assign(mat.n * pp.m_ext, Fr::zero());
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; t++)
      pool.emplace_back([&, t]() {
        std::vector<Fr> cw;
        for (size_t r = t; r < mat.n; r += threads) {
          (void)encode_host(mat.entries.data() + r * mat.m, mat.m, pp, cw);
          memcpy(ext.entries.data() + r * pp.m_ext, cw.data(), pp.m_ext * 32);
        }
      });
    for (auto& th : pool) th.join();
  }
  // encode on the device: rows x m -> rows x m_ext (one row: LinearEncode::encode; all rows: compute_matrices)
  static Error encode(pc_ctx* ctx, const pc_lincode* code, const Matrix<E>& mat, Matrix<E>& ext) {
    ext.n = mat.n; ext.m = pc_hip_brakedown_codeword_len(code); ext.entries.assign(ext.n * ext.m, Fr::zero());
    const int rc = pc_hip_brakedown_encode(ctx, code, mat.entries.data(), PC_MEM_HOST, mat.n, ext.entries.data(), PC_MEM_HOST);
    if (rc != PC_OK) { Error e; e.kind = Error::Backend; e.msg = pc_hip_strerror(rc); return e; }
    return Error();
  }
  // tensor_vec (linear_codes/utils.rs:240-258) and MultilinearBrakedown::tensor (mod.rs:96-107): the point split at log2(left_len)
  static std::vector<Fr> tensor_vec(const Fr* values, size_t count) {
    std::vector<Fr> layer{Fr::one()};
    for (size_t i = 0; i < count; i++) {
      const Fr anti = Fr::one() - values[i];
      std::vector<Fr> next; next.reserve(layer.size() * 2);
      for (const Fr& v : layer) next.push_back(v * anti);
      for (const Fr& v : layer) next.push_back(v * values[i]);
      layer.swap(next);
    }
    return layer;
  }
  static void tensor(const std::vector<Fr>& point, size_t left_len, std::vector<Fr>& a, std::vector<Fr>& b) {
    const size_t split = ark_log2(left_len);
    a = tensor_vec(point.data(), split); b = tensor_vec(point.data() + split, point.size() - split);
  }
};

// LinearCodePCS<MultilinearBrakedown>: commit / open / check for one polynomial given by its evaluations (poly_to_vec, mod.rs:86-88).
// The sponge is the caller's: the query indices (t = params.num_queries() of them) and the vector r are arguments.
template <class E>
struct BrakedownPCS : LinearCodePCS<E> {
  typedef FrT<E> Fr;
  typedef typename LinearCodePCS<E>::ProofSingle ProofSingle;
  static Error backend(int rc) { Error e; e.kind = Error::Backend; e.msg = pc_hip_strerror(rc); return e; }
  Error commit(pc_ctx* ctx, const pc_lincode* code, const BrakedownPCParams<E>& pp, const std::vector<Fr>& evals, LinCodePCCommitment& com,
               LinCodePCCommitmentState<E>& state) const {
    if (evals.size() > pp.n * pp.m || pc_hip_brakedown_codeword_len(code) != pp.m_ext) { Error e; e.kind = Error::IncorrectInputLength; e.msg = "polynomial larger than the parameters' matrix"; return e; }
    state.mat.n = pp.n; state.mat.m = pp.m; state.mat.entries = evals; state.mat.entries.resize(pp.n * pp.m, Fr::zero());
    state.ext_mat.n = pp.n; state.ext_mat.m = pp.m_ext; state.ext_mat.entries.assign(pp.n * pp.m_ext, Fr::zero());
    size_t padded = 2; while (padded < pp.m_ext) padded <<= 1;
    state.leaves.assign(pp.m_ext * 32, 0); state.nodes.assign((padded - 1) * 32, 0);
    const int rc = pc_hip_brakedown_commit(ctx, code, state.mat.entries.data(), PC_MEM_HOST, pp.n, this->col_hash, this->tree_hash, this->len_prefix ? 1 : 0,
                                           state.ext_mat.entries.data(), PC_MEM_HOST, state.leaves.data(), state.nodes.data());
    if (rc != PC_OK) return backend(rc);
    com.metadata.n_rows = pp.n; com.metadata.n_cols = pp.m; com.metadata.n_ext_cols = pp.m_ext;
    memcpy(com.root, state.nodes.data(), 32);
    return Error();
  }
  Error open(pc_ctx* ctx, const LinCodePCCommitment& com, const LinCodePCCommitmentState<E>& st, const std::vector<Fr>& point,
             const std::vector<size_t>& indices, const std::vector<Fr>* r, ProofSingle& proof) const {
    std::vector<Fr> a, b; MultilinearBrakedown<E>::tensor(point, com.metadata.n_cols, a, b);
    return this->open_tensored(ctx, st, b, indices, r, proof);
  }
  Error check(pc_ctx* ctx, const pc_lincode* code, const LinCodePCCommitment& com, const std::vector<Fr>& point, const Fr& value, const ProofSingle& proof,
              const std::vector<size_t>& indices, const std::vector<Fr>* r, bool& ok) const {
    std::vector<Fr> a, b; MultilinearBrakedown<E>::tensor(point, com.metadata.n_cols, a, b);
    if (com.metadata.n_ext_cols != pc_hip_brakedown_codeword_len(code)) return this->invalid_commitment("codeword length");
    return this->check_tensored(ctx, com, a, b, value, proof, indices, r, ok, false, [&](const std::vector<Fr>& v, std::vector<Fr>& w) {
      Matrix<E> in, out; in.n = 1; in.m = v.size(); in.entries = v;
      Error e = MultilinearBrakedown<E>::encode(ctx, code, in, out); w = out.entries; return e; });
  }
};

}  // namespace pc_host
