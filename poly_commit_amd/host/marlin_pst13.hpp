// C++ host mirror of the reference's MarlinPST13 (poly-commit/src/marlin/marlin_pst13_pc), above the C ABI (include/pc_hip.h), in
// the style of host/streaming_kzg.hpp and host/multilinear_pc.hpp: the reference's names, return shapes and errors; every MSM, the
// division and the combination of polynomials run on the device against resident keys in the dense lexicographic layout of
// pc_hip.h ("MarlinPST13").
//
//   pc_host::pst13::MarlinPST13<E>::setup      mod.rs:156-260, from a given trapdoor (betas, g, gamma_g, h)
//   ...::trim                                  :266-317
//   ...::commit                                :320-416
//   ...::open                                  :419-512
//
// What differs from the reference, and why:
//   - the key is not a BTreeMap: powers_of_g is a resident pc_srs whose point rank(e) is (prod beta_j^e_j) g (vk.g is point 0), the
//     hiding key a second small resident pc_srs, [gamma_g, then for every variable j its beta_j^t gamma_g, t = 1 .. degree + 1];
//   - randomness is an input, as in the other mirrors: setup takes the trapdoor, commit the blinding coefficients, open the
//     challenges (the sponge stays with the caller, as in host/marlin_kzg10.hpp);
//   - the blinding polynomial is a sum of univariates (the reference's "implicit assumption", mod.rs:383 and :486): a constant and,
//     per variable, the degrees 1 .. hiding_bound + 1 (Randomness::calculate_hiding_polynomial_degree).  check_hiding_bound is
//     applied to that DEGREE, as kzg10 applies it (kzg10/mod.rs:405-421): a hiding bound of supported_degree is HidingBoundToolarge
//     -- one stricter than mod.rs:373, which passes the bound itself --, so every hiding witness has at most supported_degree terms;
//   - beta_h needs G2: pc_hip_g2_point_mul is BLS12-381 only.  For every other curve (and with h == NULL) the verifier key's G2 part
//     is the caller's and beta_h stays empty;
//   - check (the verifier, mod.rs:516-558) is not built: the library has no pairing.  Trimming the number of variables, a
//     gathered-base commit for very sparse polynomials and a multi-device form are not built either.
#pragma once
#include "kzg10.hpp"

namespace pc_host {
namespace pst13 {

template <class E>
inline Error backend_error(pc_ctx* ctx, int rc) {
  Error e; e.kind = Error::Backend; e.msg = std::string(pc_hip_strerror(rc)) + ": " + pc_hip_last_error(ctx); return e;
}
template <class E>
inline G1Affine<E> point_of(const uint64_t* xy, int inf) { return G1Affine<E>::from_xy(xy, inf != 0); }

// SparsePolynomial<Fr, SparseTerm> as flat arrays: term t is coeffs[t] * prod_j X_j^exps[t * num_vars + j]
template <class E>
struct SparsePolynomial {
  size_t num_vars = 0;
  std::vector<uint8_t> exps; std::vector<FrT<E>> coeffs;
  void push(const FrT<E>& c, const std::vector<uint8_t>& e) { coeffs.push_back(c); exps.insert(exps.end(), e.begin(), e.end()); }
  size_t degree() const {
    size_t d = 0;
    for (size_t t = 0; t < coeffs.size(); t++) { size_t s = 0; for (size_t j = 0; j < num_vars; j++) s += exps[t * num_vars + j]; if (!coeffs[t].is_zero()) d = std::max(d, s); }
    return d;
  }
};
template <class E>
struct LabeledPolynomial { std::string label; SparsePolynomial<E> polynomial; bool has_hiding_bound = false; size_t hiding_bound = 0; };

// the blinding polynomial c_0 + sum_j sum_{t = 1 .. degree} c[1 + j degree + t - 1] X_j^t; degree 0: empty (not hiding)
template <class E>
struct Randomness {
  size_t num_vars = 0, degree = 0;
  std::vector<FrT<E>> coeffs;
  static Randomness empty() { return Randomness(); }
  bool is_hiding() const { for (auto& c : coeffs) if (!c.is_zero()) return true; return false; }
  static size_t calculate_hiding_polynomial_degree(size_t hiding_bound) { return hiding_bound + 1; }      // data_structures.rs:361-363
  FrT<E> coeff(size_t var, size_t t) const { return t <= degree ? coeffs[1 + var * degree + t - 1] : FrT<E>::zero(); }
  FrT<E> evaluate(const std::vector<FrT<E>>& z) const {
    if (coeffs.empty()) return FrT<E>::zero();
    FrT<E> acc = coeffs[0];
    for (size_t j = 0; j < num_vars; j++) { FrT<E> u = FrT<E>::zero(); for (size_t t = degree; t >= 1; t--) u = (u + coeff(j, t)) * z[j]; acc = acc + u; }
    return acc;
  }
};

template <class E> struct PstCommitment { G1Affine<E> comm = G1Affine<E>::zero(); };
template <class E> struct PstProof { std::vector<G1Affine<E>> w; bool has_random_v = false; FrT<E> random_v = FrT<E>::zero(); };      // data_structures.rs: Proof { w, random_v }

template <class E>
struct UniversalParams {
  pc_ctx* ctx = nullptr; size_t num_vars = 0, max_degree = 0;
  pc_srs* powers_of_g = nullptr;            // N(num_vars, max_degree) points in device order
  pc_srs* powers_of_gamma_g = nullptr;      // 1 + num_vars (max_degree + 1) points: gamma_g, then per variable beta^1 .. beta^(max_degree + 1)
  G1Affine<E> g, gamma_g;
  std::vector<uint64_t> h; std::vector<std::vector<uint64_t>> beta_h;      // G2, 4 Fq each (BLS12-381 with h given; else empty)
  void release() { pc_hip_srs_free(powers_of_g); pc_hip_srs_free(powers_of_gamma_g); powers_of_g = powers_of_gamma_g = nullptr; }
};
template <class E>
struct CommitterKey {
  pc_ctx* ctx = nullptr; size_t num_vars = 0, supported_degree = 0, max_degree = 0;
  pc_srs* powers_of_g = nullptr; pc_srs* powers_of_gamma_g = nullptr;
  G1Affine<E> gamma_g;
  size_t hiding_len() const { return 1 + num_vars * (supported_degree + 1); }
  size_t hiding_slot(size_t var, size_t t) const { return t ? 1 + var * (supported_degree + 1) + t - 1 : 0; }      // the point of X_var^t (mod.rs:385-388)
  void release() { pc_hip_srs_free(powers_of_g); pc_hip_srs_free(powers_of_gamma_g); powers_of_g = powers_of_gamma_g = nullptr; }
};
template <class E>
struct VerifierKey {
  G1Affine<E> g, gamma_g; std::vector<uint64_t> h; std::vector<std::vector<uint64_t>> beta_h;
  size_t num_vars = 0, supported_degree = 0, max_degree = 0;
};

template <class E>
struct MarlinPST13 {
  typedef FrT<E> Fr;

  static Error check_hiding_bound(size_t hiding_poly_degree, size_t num_powers) {                            // mod.rs:95-109
    Error e;
    if (hiding_poly_degree == 0) { e.kind = Error::HidingBoundIsZero; return e; }
    if (hiding_poly_degree >= num_powers) { e.kind = Error::HidingBoundToolarge; e.a = hiding_poly_degree; e.b = num_powers; return e; }
    return e;
  }
  static Error check_degrees_and_bounds(size_t supported_degree, const LabeledPolynomial<E>& p) {           // mod.rs:112-128
    Error e;
    if (p.polynomial.degree() > supported_degree) { e.kind = Error::PolynomialDegreeTooLarge; e.a = p.polynomial.degree(); e.b = supported_degree; e.msg = p.label; }
    return e;
  }

  // the hiding key of (n, d) from its scalars on the host: 1 + n (d + 1) fixed-base multiplications of gamma_g (mod.rs:219-232)
  static int make_hiding_key(pc_ctx* ctx, size_t n, size_t d, const std::vector<Fr>& betas, const G1Affine<E>& gamma_g, pc_srs** out) {
    const size_t len = 1 + n * (d + 1), pb = 16 * E::NQ;
    std::vector<Fr> s(len); s[0] = Fr::one();
    for (size_t j = 0; j < n; j++) { Fr cur = Fr::one(); for (size_t t = 0; t <= d; t++) { cur = cur * betas[j]; s[1 + j * (d + 1) + t] = cur; } }
    void* sd = nullptr; void* pts = nullptr;
    uint64_t gxy[2 * E::NQ]; gamma_g.to_xy(gxy);
    int rc = pc_hip_malloc(ctx, len * 32, &sd);
    if (rc == PC_OK) rc = pc_hip_malloc(ctx, len * pb, &pts);
    if (rc == PC_OK) rc = pc_hip_memcpy_h2d(ctx, sd, s.data(), len * 32);
    if (rc == PC_OK) rc = pc_hip_fixed_base_batch_mul(ctx, E::ID, gxy, sd, len, pts);
    if (rc == PC_OK) rc = pc_hip_srs_upload(ctx, E::ID, pts, len, 0, PC_MEM_DEVICE, out);
    if (pts) pc_hip_free(ctx, pts);
    if (sd) pc_hip_free(ctx, sd);
    return rc;
  }

  // h_g2: 4 Fq (x.c0, x.c1, y.c0, y.c1) or NULL
  static Error setup(pc_ctx* ctx, size_t max_degree, size_t num_vars, const std::vector<Fr>& betas, const G1Affine<E>& g, const G1Affine<E>& gamma_g,
                     const uint64_t* h_g2, UniversalParams<E>& pp) {
    pp = UniversalParams<E>();
    Error e;
    if (num_vars < 1 || betas.size() != num_vars) { e.kind = Error::InvalidNumberOfVariables; return e; }   // mod.rs:161-164
    if (max_degree < 1) { e.kind = Error::InvalidParameters; return e; }                                     // DegreeIsZero (:165-167)
    const size_t M = pc_hip_pst13_key_len(num_vars, max_degree), pb = 16 * E::NQ;
    if (!M) { e.kind = Error::InvalidParameters; e.a = num_vars; e.b = max_degree; return e; }
    pp.ctx = ctx; pp.num_vars = num_vars; pp.max_degree = max_degree; pp.g = g; pp.gamma_g = gamma_g;
    void* ev = nullptr; void* pts = nullptr;
    uint64_t gxy[2 * E::NQ]; g.to_xy(gxy);
    int rc = pc_hip_malloc(ctx, M * 32, &ev);
    if (rc == PC_OK) rc = pc_hip_malloc(ctx, M * pb, &pts);
    if (rc == PC_OK) rc = pc_hip_pst13_monomial_evals(ctx, E::ID, num_vars, max_degree, betas.data(), ev);   // powers_of_beta (:187-207)
    if (rc == PC_OK) rc = pc_hip_fixed_base_batch_mul(ctx, E::ID, gxy, ev, M, pts);                          // g.batch_mul (:210)
    if (rc == PC_OK) rc = pc_hip_srs_upload(ctx, E::ID, pts, M, 0, PC_MEM_DEVICE, &pp.powers_of_g);
    if (pts) pc_hip_free(ctx, pts);
    if (ev) pc_hip_free(ctx, ev);
    if (rc == PC_OK) rc = make_hiding_key(ctx, num_vars, max_degree, betas, gamma_g, &pp.powers_of_gamma_g);
    if (rc == PC_OK && h_g2 && E::ID == PC_CURVE_BLS12_381) {
      pp.h.assign(h_g2, h_g2 + 4 * E::NQ);
      pp.beta_h.assign(num_vars, std::vector<uint64_t>(4 * E::NQ));
      for (size_t j = 0; j < num_vars && rc == PC_OK; j++) rc = pc_hip_g2_point_mul(E::ID, h_g2, betas[j].l, pp.beta_h[j].data());      // :236
    }
    if (rc != PC_OK) { pp.release(); return backend_error<E>(ctx, rc); }
    return Error();
  }

  static Error trim(const UniversalParams<E>& pp, size_t supported_degree, CommitterKey<E>& ck, VerifierKey<E>& vk) {
    ck = CommitterKey<E>(); vk = VerifierKey<E>();
    if (supported_degree > pp.max_degree || !supported_degree) { Error e; e.kind = Error::TrimmingDegreeTooLarge; return e; }      // :272-275
    const size_t n = pp.num_vars, pb = 16 * E::NQ;
    ck.ctx = pp.ctx; ck.num_vars = n; ck.supported_degree = supported_degree; ck.max_degree = pp.max_degree; ck.gamma_g = pp.gamma_g;
    int rc = pc_hip_pst13_trim(pp.ctx, pp.powers_of_g, 0, n, pp.max_degree, supported_degree, &ck.powers_of_g);                     // :283-288
    if (rc == PC_OK) {                                                                                                               // e[..=supported_degree] (:289-293)
      const size_t full = 1 + n * (pp.max_degree + 1);
      std::vector<uint64_t> all(full * 2 * E::NQ), kept(ck.hiding_len() * 2 * E::NQ);
      rc = pc_hip_srs_read(pp.ctx, pp.powers_of_gamma_g, 0, full, all.data());
      if (rc == PC_OK) {
        memcpy(kept.data(), all.data(), pb);
        for (size_t j = 0; j < n; j++)
          memcpy(&kept[(1 + j * (supported_degree + 1)) * 2 * E::NQ], &all[(1 + j * (pp.max_degree + 1)) * 2 * E::NQ], (supported_degree + 1) * pb);
      }
      if (rc == PC_OK) rc = pc_hip_srs_upload(pp.ctx, E::ID, kept.data(), ck.hiding_len(), 0, PC_MEM_HOST, &ck.powers_of_gamma_g);
    }
    if (rc != PC_OK) { ck.release(); return backend_error<E>(pp.ctx, rc); }
    vk.g = pp.g; vk.gamma_g = pp.gamma_g; vk.h = pp.h; vk.beta_h = pp.beta_h;
    vk.num_vars = n; vk.supported_degree = supported_degree; vk.max_degree = pp.max_degree;
    return Error();
  }

  // an MSM on the hiding key of a vector in its layout
  static Error hiding_msm(const CommitterKey<E>& ck, const std::vector<Fr>& v, G1Affine<E>& out) {
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_msm(ck.ctx, ck.powers_of_gamma_g, 0, v.data(), PC_SCALARS_MONTGOMERY, PC_MEM_HOST, v.size(), xy, &inf);
    if (rc != PC_OK) return backend_error<E>(ck.ctx, rc);
    out = point_of<E>(xy, inf); return Error();
  }

  // blinding[i]: the 1 + num_vars (hiding_bound + 1) coefficients of polynomial i's blinding polynomial (unused without a hiding bound)
  static Error commit(const CommitterKey<E>& ck, const std::vector<const LabeledPolynomial<E>*>& polynomials, const std::vector<std::vector<Fr>>& blinding,
                      std::vector<PstCommitment<E>>& commitments, std::vector<Randomness<E>>& randomness) {
    commitments.clear(); randomness.clear();
    for (size_t i = 0; i < polynomials.size(); i++) {
      const LabeledPolynomial<E>& p = *polynomials[i];
      if (p.polynomial.num_vars != ck.num_vars) { Error e; e.kind = Error::InvalidNumberOfVariables; return e; }
      if (Error e = check_degrees_and_bounds(ck.supported_degree, p)) return e;                                                       // :342
      uint64_t xy[2 * E::NQ]; int inf = 0;
      int rc = pc_hip_pst13_commit(ck.ctx, ck.powers_of_g, 0, ck.num_vars, ck.supported_degree, nullptr, PC_MEM_HOST, p.polynomial.exps.data(),
                                   p.polynomial.coeffs.data(), PC_MEM_HOST, p.polynomial.coeffs.size(), xy, &inf);                     // :353-362
      if (rc != PC_OK) return backend_error<E>(ck.ctx, rc);
      G1Affine<E> commitment = point_of<E>(xy, inf);
      Randomness<E> rand = Randomness<E>::empty();
      if (p.has_hiding_bound) {
        const size_t deg = Randomness<E>::calculate_hiding_polynomial_degree(p.hiding_bound);
        if (Error e = check_hiding_bound(deg, ck.supported_degree + 1)) return e;                                                    // :373, on the degree (see the head)
        if (i >= blinding.size() || blinding[i].size() != 1 + ck.num_vars * deg) { Error e; e.kind = Error::MissingRng; return e; }
        rand.num_vars = ck.num_vars; rand.degree = deg; rand.coeffs = blinding[i];
        std::vector<Fr> v(ck.hiding_len(), Fr::zero());                                                                               // :377-399
        v[0] = rand.coeffs[0];
        for (size_t j = 0; j < ck.num_vars; j++) for (size_t t = 1; t <= deg; t++) v[ck.hiding_slot(j, t)] = rand.coeff(j, t);
        G1Affine<E> random_commitment;
        if (Error e = hiding_msm(ck, v, random_commitment)) return e;
        commitment = commitment.add(random_commitment);                                                                              // :403
      }
      PstCommitment<E> c; c.comm = commitment;
      commitments.push_back(c); randomness.push_back(rand);
    }
    return Error();
  }

  // challenges[j]: the sponge's challenge_j of polynomial j (:440)
  static Error open(const CommitterKey<E>& ck, const std::vector<const LabeledPolynomial<E>*>& labeled_polynomials, const std::vector<Fr>& point,
                    const std::vector<Fr>& challenges, const std::vector<const Randomness<E>*>& states, PstProof<E>& proof) {
    proof = PstProof<E>();
    const size_t n = ck.num_vars, d = ck.supported_degree, k = labeled_polynomials.size();
    if (point.size() != n) { Error e; e.kind = Error::InvalidNumberOfVariables; return e; }
    if (!k || challenges.size() < k || states.size() < k) { Error e; e.kind = Error::IncorrectInputLength; return e; }
    for (size_t j = 0; j < k; j++) {
      if (labeled_polynomials[j]->polynomial.num_vars != n) { Error e; e.kind = Error::InvalidNumberOfVariables; return e; }
      if (Error e = check_degrees_and_bounds(d, *labeled_polynomials[j])) return e;                                                  // :437
    }
    // p = sum challenge_j p_j on dense device vectors (:442); r likewise on the host (:443), in the hiding key's layout
    const size_t M = pc_hip_pst13_key_len(n, d);
    std::vector<void*> dense(k + 1, nullptr);
    int rc = PC_OK;
    for (size_t j = 0; j <= k && rc == PC_OK; j++) rc = pc_hip_malloc(ck.ctx, M * 32, &dense[j]);
    for (size_t j = 0; j < k && rc == PC_OK; j++) {
      const SparsePolynomial<E>& q = labeled_polynomials[j]->polynomial;
      rc = pc_hip_pst13_scatter(ck.ctx, E::ID, n, d, q.exps.data(), q.coeffs.data(), PC_MEM_HOST, q.coeffs.size(), dense[j]);
    }
    std::vector<size_t> lens(k, M);
    if (rc == PC_OK) rc = pc_hip_fr_lincomb(ck.ctx, E::ID, dense.data(), PC_MEM_DEVICE, lens.data(), k, challenges.data(), dense[k], PC_MEM_DEVICE, M);
    std::vector<uint64_t> xy(n * 2 * E::NQ); std::vector<int> inf(n); Fr value;
    if (rc == PC_OK) rc = pc_hip_pst13_open(ck.ctx, ck.powers_of_g, 0, n, d, dense[k], PC_MEM_DEVICE, nullptr, nullptr, PC_MEM_HOST, 0, point.data(),
                                            xy.data(), inf.data(), value.l);                                                          // :448, :457-469
    for (void* p : dense) if (p) pc_hip_free(ck.ctx, p);
    if (rc != PC_OK) return backend_error<E>(ck.ctx, rc);
    proof.w.resize(n);
    for (size_t i = 0; i < n; i++) proof.w[i] = point_of<E>(&xy[i * 2 * E::NQ], inf[i]);

    Randomness<E> r; r.num_vars = n;
    for (size_t j = 0; j < k; j++) r.degree = std::max(r.degree, states[j]->degree);
    r.coeffs.assign(r.degree ? 1 + n * r.degree : 0, Fr::zero());
    for (size_t j = 0; j < k; j++) {
      const Randomness<E>& s = *states[j];
      if (s.coeffs.empty()) continue;
      r.coeffs[0] = r.coeffs[0] + challenges[j] * s.coeffs[0];
      for (size_t v = 0; v < n; v++) for (size_t t = 1; t <= s.degree; t++) r.coeffs[1 + v * r.degree + t - 1] = r.coeffs[1 + v * r.degree + t - 1] + challenges[j] * s.coeff(v, t);
    }
    if (r.is_hiding()) {                                                                                                              // :449-453, :474-506
      // divide_at_point of a sum of univariates: pass i meets only u_i(X_i); w_i = (u_i - u_i(z_i)) / (X_i - z_i), at most d terms
      for (size_t i = 0; i < n; i++) {
        std::vector<Fr> v(ck.hiding_len(), Fr::zero());
        Fr acc = Fr::zero();
        for (size_t t = r.degree; t >= 1; t--) { acc = r.coeff(i, t) + point[i] * acc; v[ck.hiding_slot(i, t - 1)] = acc; }                     // q[t - 1] = c[t] + z q[t]
        G1Affine<E> hw;
        if (Error e = hiding_msm(ck, v, hw)) return e;
        proof.w[i] = proof.w[i].add(hw);                                                                                             // :497-500
      }
      proof.has_random_v = true; proof.random_v = r.evaluate(point);                                                                 // :503
    }
    return Error();
  }
};

}  // namespace pst13
}  // namespace pc_host
