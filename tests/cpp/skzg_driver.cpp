// Driver of host/streaming_kzg.hpp: the reference's own consistency checks (streaming_kzg/tests.rs) through the C++ mirror.
//   - time and space forms give equal commitments and proofs (tests.rs:40-83);
//   - for one point the multi-point proof equals the single-point proof, the remainder is the evaluation (tests.rs:228-239);
//   - the remainder of a multi-point opening evaluates like the polynomial at the points (tests.rs:241-251);
//   - commit_folding's first level is the commitment of the polynomial folded on the host; open_folding's remainders evaluate like
//     the levels.
// Exit 77 with "no HIP device" where there is none (the CPU suite compiles and links this file; the GPU suite runs it).
#include <stdio.h>
#include "../../poly_commit_amd/host/streaming_kzg.hpp"

using namespace pc_host;
typedef Bls12_381 E;
typedef FrT<E> Fr;

static Fr eval_be(const std::vector<Fr>& high_first, const Fr& x) { Fr a = Fr::zero(); for (auto& c : high_first) a = a * x + c; return a; }
static Fr eval_le(const std::vector<Fr>& low_first, const Fr& x) { Fr a = Fr::zero(); for (size_t i = low_first.size(); i-- > 0;) a = a * x + low_first[i]; return a; }
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define NOERR(e) do { Error _e = (e); if (_e) { printf("FAILED line %d: error %d %s\n", __LINE__, (int)_e.kind, _e.msg.c_str()); return 1; } } while (0)

int main() {
  pc_ctx* ctx = nullptr;
  int rc = pc_hip_init(0, &ctx);
  if (rc == PC_ERR_NO_DEVICE) { printf("no HIP device\n"); return 77; }
  if (rc != PC_OK) { printf("init failed: %s\n", pc_hip_strerror(rc)); return 1; }
  uint64_t seed = 0x5C26;
  auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return Fr::from_u64(seed >> 11) * Fr::from_u64(seed | 1); };
  uint64_t gxy[2 * E::NQ];
  memcpy(gxy, E::C::GX, 8 * E::NQ); memcpy(gxy + E::NQ, E::C::GY, 8 * E::NQ);
  const G1Affine<E> g = G1Affine<E>::from_xy(gxy, false);
  const size_t max_degree = 300, max_eval_points = 5;
  skzg::CommitterKey<E> ck;
  NOERR(skzg::CommitterKey<E>::make(ctx, max_degree, max_eval_points, next(), g, nullptr, ck));
  skzg::CommitterKeyStream<E> sck(ck);
  CHECK(ck.max_eval_points() == 5);

  std::vector<Fr> poly(101); for (auto& c : poly) c = next();
  Commitment<E> c_time, c_space;
  NOERR(ck.commit(poly, c_time)); NOERR(sck.commit(poly, c_space));
  CHECK(c_time.comm == c_space.comm && !c_time.comm.is_zero());

  const Fr beta = next();
  Fr ev_t, ev_s; skzg::EvaluationProof<E> p_t, p_s, p_m;
  NOERR(ck.open(poly, beta, ev_t, p_t)); NOERR(sck.open(poly, beta, 1 << 20, ev_s, p_s));
  CHECK(ev_t == ev_s && ev_t == eval_le(poly, beta) && p_t.w == p_s.w);
  std::vector<Fr> rem;
  NOERR(sck.open_multi_points(poly, {beta}, 1 << 20, rem, p_m));
  CHECK(rem.size() == 1 && rem[0] == ev_t && p_m.w == p_t.w);

  const std::vector<Fr> pts = {beta, beta.neg(), beta * beta};
  skzg::EvaluationProof<E> pm_t, pm_s;
  NOERR(ck.open_multi_points(poly, pts, pm_t)); NOERR(sck.open_multi_points(poly, pts, 1 << 20, rem, pm_s));
  CHECK(pm_t.w == pm_s.w && rem.size() == 3);
  for (auto& z : pts) CHECK(eval_be(rem, z) == eval_le(poly, z));
  std::vector<Fr> tiny(3, Fr::one());
  NOERR(ck.open_multi_points(tiny, pts, pm_t)); CHECK(pm_t.w.is_zero());                                  // at most k coefficients: the identity
  CHECK(sck.open_multi_points(std::vector<Fr>(2, Fr::one()), pts, 0, rem, pm_s).kind == Error::IncorrectInputLength);

  // batch: eta-combination on the host, then the single-polynomial opening
  std::vector<Fr> other(40); for (auto& c : other) c = next();
  const Fr eta = next();
  std::vector<Fr> comb = poly; for (size_t i = 0; i < other.size(); i++) comb[i] = comb[i] + eta * other[i];
  skzg::EvaluationProof<E> pb, pc_;
  NOERR(ck.batch_open_multi_points({&poly, &other}, pts, eta, pb)); NOERR(ck.open_multi_points(comb, pts, pc_));
  CHECK(pb.w == pc_.w);
  CHECK(ck.batch_open_multi_points({&poly}, std::vector<Fr>(6, beta), eta, pb).kind == Error::InvalidParameters);      // time.rs:147

  // folding: every level on the host
  const size_t depth = 7;
  std::vector<Fr> rhos(depth), etas(depth); for (auto& c : rhos) c = next(); for (auto& c : etas) c = next();
  std::vector<std::vector<Fr>> levels; std::vector<Fr> cur = poly;
  for (size_t i = 0; i < depth; i++) {
    std::vector<Fr> nx((cur.size() + 1) / 2);
    for (size_t b = 0; b < nx.size(); b++) nx[b] = 2 * b + 1 < cur.size() ? cur[2 * b] + rhos[i] * cur[2 * b + 1] : cur[2 * b];
    levels.push_back(nx); cur = nx;
  }
  std::vector<Commitment<E>> cf;
  NOERR(sck.commit_folding(poly, rhos, 1 << 20, cf));
  CHECK(cf.size() == depth);
  for (size_t i = 0; i < depth; i++) { Commitment<E> c; NOERR(ck.commit(levels[i], c)); CHECK(cf[i].comm == c.comm); }
  std::vector<std::vector<Fr>> rems; skzg::EvaluationProof<E> pf;
  NOERR(sck.open_folding(poly, rhos, pts, etas, 1 << 20, rems, pf));
  CHECK(rems.size() == depth && !pf.w.is_zero());
  for (size_t i = 0; i < depth; i++) for (auto& z : pts) CHECK(eval_be(rems[i], z) == eval_le(levels[i], z));
  // the proof is the eta-combination of the levels' own multi-point proofs
  G1Affine<E> want = G1Affine<E>::zero();
  for (size_t i = 0; i < depth; i++) { skzg::EvaluationProof<E> pi; NOERR(ck.open_multi_points(levels[i], pts, pi)); want = want.add(pi.w.mul(etas[i])); }
  CHECK(pf.w == want);

  ck.release();
  pc_hip_shutdown(ctx);
  printf("streaming_kzg host mirror OK\n");
  return 0;
}
