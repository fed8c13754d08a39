// C++ host mirror of the reference's streaming_kzg (poly-commit/src/streaming_kzg), above the C ABI (include/pc_hip.h), in the
// style of host/kzg10.hpp: the reference's names, return shapes and asserts (as error returns); every MSM, division and fold runs on
// the device against ONE resident key.
//
//   pc_host::skzg::CommitterKey<E>::make                        streaming_kzg/time.rs:44-63 (`new`, from a given tau, g, g2)
//   ...::commit / batch_commit                                  :72-74, :90-99
//   ...::open                                                   :104-123
//   ...::open_multi_points / batch_open_multi_points            :126-137, :141-152
//   pc_host::skzg::CommitterKeyStream<E>::commit / open         streaming_kzg/space.rs:139-149, :65-95
//   ...::open_multi_points                                      :98-136
//   ...::commit_folding / open_folding                          :165-199, :205-262
//
// The reference's space form reads streams, HIGHEST degree first, against the reversed key, in bounded memory; here a "stream" is a
// coefficient vector in natural order (index = degree: a caller that holds a stream reverses it once) and `max_msm_buffer` is
// accepted and ignored -- the key and the polynomial are resident.  Remainders come back as the reference returns them: highest
// degree first.  index_by and the verifier (VerifierKey::verify*, pairings) are not built.
#pragma once
#include "kzg10.hpp"

namespace pc_host {
namespace skzg {

template <class E> struct EvaluationProof { G1Affine<E> w = G1Affine<E>::zero(); };       // EvaluationProof(pub E::G1Affine)

template <class E>
inline Error backend_error(pc_ctx* ctx, int rc) {
  Error e; e.kind = Error::Backend; e.msg = std::string(pc_hip_strerror(rc)) + ": " + pc_hip_last_error(ctx); return e;
}
template <class E>
inline G1Affine<E> point_of(const uint64_t* xy, int inf) { return G1Affine<E>::from_xy(xy, inf != 0); }

template <class E>
struct CommitterKey {
  typedef FrT<E> Fr;
  pc_ctx* ctx = nullptr;
  pc_srs* powers_of_g = nullptr; size_t n_powers = 0;       // resident: tau^d g, d <= max_degree
  std::vector<uint64_t> powers_of_g2; size_t n_g2 = 0;      // host: tau^d g2, d <= max_eval_points, 4 Fq each (BLS12-381; else only counted)

  // `new` with the trapdoor handed in (the reference draws tau, g, g2 from its rng, time.rs:46-52): powers(tau, max_degree + 1) and
  // g.batch_mul on the device; g2_host may be NULL on a curve without the G2 entry points (the count of G2 powers is kept for the assert
  // of batch_open_multi_points)
  static Error make(pc_ctx* ctx, size_t max_degree, size_t max_eval_points, const Fr& tau, const G1Affine<E>& g, const void* g2_host, CommitterKey& out) {
    out = CommitterKey(); out.ctx = ctx; out.n_powers = max_degree + 1; out.n_g2 = max_eval_points + 1;
    if (max_eval_points > max_degree) { Error e; e.kind = Error::InvalidParameters; return e; }      // `take(max_eval_points + 1)` of max_degree + 1 powers
    const size_t n = out.n_powers, pb = 16 * E::NQ;
    void* pw = nullptr; void* pts = nullptr; void* pts2 = nullptr;
    uint64_t gxy[2 * E::NQ]; g.to_xy(gxy);
    int rc = pc_hip_malloc(ctx, n * 32, &pw);
    if (rc == PC_OK) rc = pc_hip_malloc(ctx, n * pb, &pts);
    if (rc == PC_OK) rc = pc_hip_fr_powers(ctx, E::ID, tau.l, n, pw);
    if (rc == PC_OK) rc = pc_hip_fixed_base_batch_mul(ctx, E::ID, gxy, pw, n, pts);
    if (rc == PC_OK) rc = pc_hip_srs_upload(ctx, E::ID, pts, n, 0, PC_MEM_DEVICE, &out.powers_of_g);
    if (rc == PC_OK && g2_host) {
      out.powers_of_g2.resize(out.n_g2 * 4 * E::NQ);
      rc = pc_hip_malloc(ctx, out.n_g2 * 2 * pb, &pts2);
      if (rc == PC_OK) rc = pc_hip_g2_fixed_base_batch_mul(ctx, E::ID, g2_host, pw, out.n_g2, pts2);
      if (rc == PC_OK) rc = pc_hip_memcpy_d2h(ctx, out.powers_of_g2.data(), pts2, out.n_g2 * 2 * pb);
    }
    if (pts2) pc_hip_free(ctx, pts2);
    if (pts) pc_hip_free(ctx, pts);
    if (pw) pc_hip_free(ctx, pw);
    if (rc != PC_OK) { out.release(); return backend_error<E>(ctx, rc); }
    return Error();
  }
  void release() { pc_hip_srs_free(powers_of_g); powers_of_g = nullptr; }
  size_t max_eval_points() const { return n_g2 - 1; }

  // msm over min(powers, coefficients) pairs, as ark's msm does
  Error commit(const std::vector<Fr>& polynomial, Commitment<E>& out) const {
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_msm(ctx, powers_of_g, 0, polynomial.data(), PC_SCALARS_MONTGOMERY, PC_MEM_HOST, polynomial.size(), xy, &inf);
    if (rc != PC_OK) return backend_error<E>(ctx, rc);
    out.comm = point_of<E>(xy, inf); return Error();
  }
  Error batch_commit(const std::vector<const std::vector<Fr>*>& polynomials, std::vector<Commitment<E>>& out) const {
    const size_t m = polynomials.size();
    std::vector<const void*> ptrs(m); std::vector<size_t> lens(m); std::vector<uint64_t> xy(m * 2 * E::NQ); std::vector<int> inf(m);
    for (size_t j = 0; j < m; j++) { ptrs[j] = polynomials[j]->data(); lens[j] = polynomials[j]->size(); }
    int rc = pc_hip_msm_batch(ctx, powers_of_g, nullptr, ptrs.data(), lens.data(), m, PC_SCALARS_MONTGOMERY, PC_MEM_HOST, xy.data(), inf.data());
    if (rc != PC_OK) return backend_error<E>(ctx, rc);
    out.resize(m);
    for (size_t j = 0; j < m; j++) out[j].comm = point_of<E>(&xy[j * 2 * E::NQ], inf[j]);
    return Error();
  }
  // (evaluation, proof); the empty polynomial gives (0, identity) (time.rs:118-121)
  Error open(const std::vector<Fr>& polynomial, const Fr& evaluation_point, Fr& evaluation, EvaluationProof<E>& proof) const {
    evaluation = Fr::zero(); proof = EvaluationProof<E>();
    if (polynomial.empty()) return Error();
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_kzg_open(ctx, powers_of_g, 0, polynomial.data(), PC_MEM_HOST, polynomial.size(), evaluation_point.l, xy, &inf);
    if (rc == PC_OK) rc = pc_hip_poly_eval(ctx, E::ID, polynomial.data(), PC_MEM_HOST, polynomial.size(), evaluation_point.l, evaluation.l);
    if (rc != PC_OK) return backend_error<E>(ctx, rc);
    proof.w = point_of<E>(xy, inf); return Error();
  }
  // a polynomial of at most eval_points.len() coefficients has the zero quotient: the identity (time.rs:134-136)
  Error open_multi_points(const std::vector<Fr>& polynomial, const std::vector<Fr>& eval_points, EvaluationProof<E>& proof) const {
    proof = EvaluationProof<E>();
    if (eval_points.empty()) { Commitment<E> c; Error e = commit(polynomial, c); proof.w = c.comm; return e; }      // Z = 1
    if (polynomial.size() <= eval_points.size()) return Error();
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_kzg_open_multi(ctx, powers_of_g, 0, polynomial.data(), PC_MEM_HOST, polynomial.size(), eval_points.data(), eval_points.size(),
                                   nullptr, xy, &inf);
    if (rc != PC_OK) return backend_error<E>(ctx, rc);
    proof.w = point_of<E>(xy, inf); return Error();
  }
  Error batch_open_multi_points(const std::vector<const std::vector<Fr>*>& polynomials, const std::vector<Fr>& eval_points, const Fr& eval_chal,
                                EvaluationProof<E>& proof) const {
    proof = EvaluationProof<E>();
    if (!(eval_points.size() < n_g2)) { Error e; e.kind = Error::InvalidParameters; e.a = eval_points.size(); e.b = n_g2; return e; }      // time.rs:147
    if (polynomials.empty() || eval_points.empty()) { Error e; e.kind = Error::IncorrectInputLength; return e; }
    const size_t m = polynomials.size();
    std::vector<const void*> ptrs(m); std::vector<size_t> lens(m);
    for (size_t j = 0; j < m; j++) { ptrs[j] = polynomials[j]->data(); lens[j] = polynomials[j]->size(); }
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_kzg_batch_open_multi(ctx, powers_of_g, 0, ptrs.data(), PC_MEM_HOST, lens.data(), m, eval_points.data(), eval_points.size(),
                                         eval_chal.l, xy, &inf);
    if (rc != PC_OK) return backend_error<E>(ctx, rc);
    proof.w = point_of<E>(xy, inf); return Error();
  }
};

// CommitterKeyStream::from(&CommitterKey) (space.rs:265-274): the same resident key
template <class E>
struct CommitterKeyStream {
  typedef FrT<E> Fr;
  const CommitterKey<E>* ck = nullptr;
  explicit CommitterKeyStream(const CommitterKey<E>& k) : ck(&k) {}

  Error commit(const std::vector<Fr>& polynomial, Commitment<E>& out) const {
    if (ck->n_powers < polynomial.size()) { Error e; e.kind = Error::TooManyCoefficients; e.a = polynomial.size(); e.b = ck->n_powers; return e; }      // space.rs:144
    return ck->commit(polynomial, out);
  }
  Error open(const std::vector<Fr>& polynomial, const Fr& alpha, size_t /*max_msm_buffer*/, Fr& evaluation, EvaluationProof<E>& proof) const {
    return ck->open(polynomial, alpha, evaluation, proof);
  }
  // (remainder highest degree first, proof); fewer coefficients than points is the reference's panic (space.rs:119-121)
  Error open_multi_points(const std::vector<Fr>& polynomial, const std::vector<Fr>& points, size_t /*max_msm_buffer*/, std::vector<Fr>& remainder,
                          EvaluationProof<E>& proof) const {
    proof = EvaluationProof<E>(); remainder.assign(points.size(), Fr::zero());
    if (points.empty() || polynomial.size() < points.size()) { Error e; e.kind = Error::IncorrectInputLength; e.a = polynomial.size(); e.b = points.size(); return e; }
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_kzg_open_multi(ck->ctx, ck->powers_of_g, 0, polynomial.data(), PC_MEM_HOST, polynomial.size(), points.data(), points.size(),
                                   remainder.data(), xy, &inf);
    if (rc != PC_OK) return backend_error<E>(ck->ctx, rc);
    proof.w = point_of<E>(xy, inf); return Error();
  }
  // one commitment per level 1 .. challenges.len() of the folding tree of `coefficients`
  Error commit_folding(const std::vector<Fr>& coefficients, const std::vector<Fr>& challenges, size_t /*max_msm_buffer*/, std::vector<Commitment<E>>& out) const {
    const size_t depth = challenges.size();
    out.clear();
    if (!depth) return Error();
    if (coefficients.empty()) { Error e; e.kind = Error::IncorrectInputLength; return e; }
    std::vector<uint64_t> xy(depth * 2 * E::NQ); std::vector<int> inf(depth);
    int rc = pc_hip_kzg_commit_folding(ck->ctx, ck->powers_of_g, 0, coefficients.data(), PC_MEM_HOST, coefficients.size(), challenges.data(), depth,
                                       xy.data(), inf.data());
    if (rc != PC_OK) return backend_error<E>(ck->ctx, rc);
    out.resize(depth);
    for (size_t i = 0; i < depth; i++) out[i].comm = point_of<E>(&xy[i * 2 * E::NQ], inf[i]);
    return Error();
  }
  // (one remainder per level, highest degree first; the one proof over the eta-combined quotients)
  Error open_folding(const std::vector<Fr>& coefficients, const std::vector<Fr>& challenges, const std::vector<Fr>& points, const std::vector<Fr>& etas,
                     size_t /*max_msm_buffer*/, std::vector<std::vector<Fr>>& remainders, EvaluationProof<E>& proof) const {
    const size_t depth = challenges.size(), k = points.size();
    proof = EvaluationProof<E>(); remainders.assign(depth, std::vector<Fr>(k, Fr::zero()));
    if (!depth) return Error();
    if (coefficients.empty() || !k || etas.size() < depth) { Error e; e.kind = Error::IncorrectInputLength; return e; }      // etas[i - 1] (space.rs:251)
    std::vector<Fr> flat(depth * k);
    uint64_t xy[2 * E::NQ]; int inf = 0;
    int rc = pc_hip_kzg_open_folding(ck->ctx, ck->powers_of_g, 0, coefficients.data(), PC_MEM_HOST, coefficients.size(), challenges.data(), depth,
                                     points.data(), k, etas.data(), flat.data(), xy, &inf);
    if (rc != PC_OK) return backend_error<E>(ck->ctx, rc);
    for (size_t i = 0; i < depth; i++) remainders[i].assign(flat.begin() + i * k, flat.begin() + (i + 1) * k);
    proof.w = point_of<E>(xy, inf); return Error();
  }
};

}  // namespace skzg
}  // namespace pc_host
