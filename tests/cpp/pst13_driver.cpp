// Driver of host/marlin_pst13.hpp: setup from a known trapdoor, trim, commit and open of two polynomials with given challenges --
// without hiding, with hiding bounds 1 and supported_degree - 1 -- through the C++ mirror.  Every input and every result is printed
// as "name: hex words" (Fr and Fq in Montgomery form, as they lie in memory), and so is every point of setup's hiding key; tests/test_pst13_gpu.py recomputes the results from the
// printed inputs with tests/harness/pst13.py.  Checked here: the reference's errors, and that a key trimmed from degree 4 to 2
// equals, point for point and in its commitments and proofs, a key set up at degree 2.
// argv[1] (optional): h, a G2 point as 24 hex words (BLS12-381) -- beta_h is then printed too.
// Exit 77 with "no HIP device" where there is none (the CPU suite compiles and links this file; the GPU suite runs it).
#include <stdio.h>
#include <stdlib.h>
#include "../../poly_commit_amd/host/marlin_pst13.hpp"

using namespace pc_host;
typedef Bls12_381 E;
typedef FrT<E> Fr;
typedef pst13::MarlinPST13<E> PC;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define NOERR(e) do { Error _e = (e); if (_e) { printf("FAILED line %d: error %d %s\n", __LINE__, (int)_e.kind, _e.msg.c_str()); return 1; } } while (0)

static void put(const char* name, const uint64_t* w, size_t n) { printf("%s:", name); for (size_t i = 0; i < n; i++) printf(" %016llx", (unsigned long long)w[i]); printf("\n"); }
static void put(const char* name, const std::vector<Fr>& v) { printf("%s:", name); for (auto& f : v) for (int i = 0; i < 4; i++) printf(" %016llx", (unsigned long long)f.l[i]); printf("\n"); }
static void put(const char* name, const G1Affine<E>& p) { uint64_t xy[2 * E::NQ]; p.to_xy(xy); put(name, xy, 2 * E::NQ); }
static void put(const char* name, const std::vector<G1Affine<E>>& v) { std::vector<uint64_t> xy(v.size() * 2 * E::NQ); for (size_t i = 0; i < v.size(); i++) v[i].to_xy(&xy[i * 2 * E::NQ]); put(name, xy.data(), xy.size()); }
static void put(const char* name, const pst13::SparsePolynomial<E>& p) {
  printf("%s_exps:", name); for (uint8_t e : p.exps) printf(" %02x", e); printf("\n");
  put((std::string(name) + "_coeffs").c_str(), p.coeffs);
}

int main(int argc, char** argv) {
  pc_ctx* ctx = nullptr;
  int rc = pc_hip_init(0, &ctx);
  if (rc == PC_ERR_NO_DEVICE) { printf("no HIP device\n"); return 77; }
  if (rc != PC_OK) { printf("init failed: %s\n", pc_hip_strerror(rc)); return 1; }
  uint64_t seed = 0x9513;
  auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return Fr::from_u64(seed >> 11) * Fr::from_u64(seed | 1); };
  uint64_t gxy[2 * E::NQ];
  memcpy(gxy, E::C::GX, 8 * E::NQ); memcpy(gxy + E::NQ, E::C::GY, 8 * E::NQ);
  const G1Affine<E> g = G1Affine<E>::from_xy(gxy, false);
  std::vector<uint64_t> h;
  if (argc > 1) { char* s = argv[1]; for (int i = 0; i < 4 * E::NQ; i++) h.push_back(strtoull(s, &s, 16)); }

  const size_t n = 3, d = 4;
  std::vector<Fr> betas(n); for (auto& b : betas) b = next();
  const Fr gamma = next();
  const G1Affine<E> gamma_g = g.mul(gamma);
  put("betas", betas); put("gamma", std::vector<Fr>{gamma});
  pst13::UniversalParams<E> pp, pp2;
  CHECK(PC::setup(ctx, d, 0, {}, g, gamma_g, nullptr, pp).kind == Error::InvalidNumberOfVariables);
  NOERR(PC::setup(ctx, d, n, betas, g, gamma_g, h.empty() ? nullptr : h.data(), pp));
  for (size_t j = 0; j < pp.beta_h.size(); j++) put("beta_h", pp.beta_h[j].data(), pp.beta_h[j].size());
  {                                                             // setup's hiding key, every point: gamma_g, then beta_j^t gamma_g, t = 1 .. d + 1
    std::vector<uint64_t> hk((1 + n * (d + 1)) * 2 * E::NQ);
    CHECK(pc_hip_srs_len(pp.powers_of_gamma_g) == 1 + n * (d + 1));
    CHECK(pc_hip_srs_read(ctx, pp.powers_of_gamma_g, 0, 1 + n * (d + 1), hk.data()) == PC_OK);
    put("hiding_key", hk.data(), hk.size());
  }
  pst13::CommitterKey<E> ck, ck2, ck_small; pst13::VerifierKey<E> vk, vk2, vk_small;
  CHECK(PC::trim(pp, d + 1, ck, vk).kind == Error::TrimmingDegreeTooLarge);
  NOERR(PC::trim(pp, d, ck, vk));
  CHECK(vk.g == g && vk.gamma_g == gamma_g && vk.num_vars == n && vk.supported_degree == d);
  { uint64_t p0[2 * E::NQ]; CHECK(pc_hip_srs_read(ctx, ck.powers_of_g, 0, 1, p0) == PC_OK); CHECK(G1Affine<E>::from_xy(p0, false) == vk.g); }      // vk.g is point 0

  // two polynomials: one with every shape of term (a repeated variable, a constant, a zero coefficient), one a sum of univariates
  pst13::LabeledPolynomial<E> a, b; a.label = "a"; b.label = "b"; a.polynomial.num_vars = b.polynomial.num_vars = n;
  a.polynomial.push(next(), {0, 0, 0}); a.polynomial.push(next(), {1, 2, 1}); a.polynomial.push(next(), {0, 0, 4}); a.polynomial.push(Fr::zero(), {2, 0, 0});
  a.polynomial.push(next(), {0, 3, 0}); a.polynomial.push(next(), {1, 0, 0});
  for (uint8_t j = 0; j < n; j++) for (uint8_t t = 1; t <= 2; t++) { std::vector<uint8_t> e(n, 0); e[j] = t; b.polynomial.push(next(), e); }
  put("a", a.polynomial); put("b", b.polynomial);
  const std::vector<Fr> point = {next(), Fr::zero(), next()}, challenges = {next(), next()};
  put("point", point); put("challenges", challenges);

  const size_t bounds[3] = {0, 1, d - 1};
  for (size_t hb : bounds) {
    a.has_hiding_bound = b.has_hiding_bound = hb != 0; a.hiding_bound = b.hiding_bound = hb;
    std::vector<std::vector<Fr>> blinding(2);
    if (hb) for (auto& v : blinding) { v.resize(1 + n * (hb + 1)); for (auto& c : v) c = next(); }
    std::vector<pst13::PstCommitment<E>> comms; std::vector<pst13::Randomness<E>> rands;
    NOERR(PC::commit(ck, {&a, &b}, blinding, comms, rands));
    pst13::PstProof<E> proof;
    NOERR(PC::open(ck, {&a, &b}, point, challenges, {&rands[0], &rands[1]}, proof));
    CHECK(proof.w.size() == n && proof.has_random_v == (hb != 0));
    char name[64];
    printf("case: %zu\n", hb);
    if (hb) { snprintf(name, sizeof name, "blinding_a"); put(name, blinding[0]); put("blinding_b", blinding[1]); }
    put("comm_a", comms[0].comm); put("comm_b", comms[1].comm); put("w", proof.w);
    if (hb) put("random_v", std::vector<Fr>{proof.random_v});
  }
  // the reference's errors
  {
    std::vector<pst13::PstCommitment<E>> comms; std::vector<pst13::Randomness<E>> rands;
    a.has_hiding_bound = true; a.hiding_bound = d;
    Error e = PC::commit(ck, {&a}, {std::vector<Fr>(1 + n * (d + 1), Fr::one())}, comms, rands);
    CHECK(e.kind == Error::HidingBoundToolarge && e.a == d + 1 && e.b == d + 1);
    a.has_hiding_bound = false;
    pst13::LabeledPolynomial<E> big = a; big.label = "big"; big.polynomial.push(Fr::one(), {2, 2, 1});
    e = PC::commit(ck, {&big}, {}, comms, rands);
    CHECK(e.kind == Error::PolynomialDegreeTooLarge && e.a == 5 && e.b == d && e.msg == "big");
  }

  // trim from 4 to 2 against a setup at 2
  NOERR(PC::trim(pp, 2, ck_small, vk_small));
  NOERR(PC::setup(ctx, 2, n, betas, g, gamma_g, nullptr, pp2));
  NOERR(PC::trim(pp2, 2, ck2, vk2));
  {
    const size_t M2 = pc_hip_pst13_key_len(n, 2), H2 = ck2.hiding_len();
    CHECK(pc_hip_srs_len(ck_small.powers_of_g) == M2 && pc_hip_srs_len(ck2.powers_of_g) == M2 && pc_hip_srs_len(ck_small.powers_of_gamma_g) == H2);
    std::vector<uint64_t> x(M2 * 2 * E::NQ), y(M2 * 2 * E::NQ), hx(H2 * 2 * E::NQ), hy(H2 * 2 * E::NQ);
    CHECK(pc_hip_srs_read(ctx, ck_small.powers_of_g, 0, M2, x.data()) == PC_OK && pc_hip_srs_read(ctx, ck2.powers_of_g, 0, M2, y.data()) == PC_OK);
    CHECK(pc_hip_srs_read(ctx, ck_small.powers_of_gamma_g, 0, H2, hx.data()) == PC_OK && pc_hip_srs_read(ctx, ck2.powers_of_gamma_g, 0, H2, hy.data()) == PC_OK);
    CHECK(x == y && hx == hy);
    b.has_hiding_bound = true; b.hiding_bound = 1;
    std::vector<std::vector<Fr>> blinding(1, std::vector<Fr>(1 + n * 2)); for (auto& c : blinding[0]) c = next();
    std::vector<pst13::PstCommitment<E>> c1, c2; std::vector<pst13::Randomness<E>> r1, r2; pst13::PstProof<E> p1, p2;
    NOERR(PC::commit(ck_small, {&b}, blinding, c1, r1)); NOERR(PC::commit(ck2, {&b}, blinding, c2, r2));
    NOERR(PC::open(ck_small, {&b}, point, challenges, {&r1[0]}, p1)); NOERR(PC::open(ck2, {&b}, point, challenges, {&r2[0]}, p2));
    CHECK(c1[0].comm == c2[0].comm && !c1[0].comm.is_zero() && p1.w == p2.w && p1.random_v == p2.random_v);
    Error e = PC::commit(ck_small, {&a}, {}, c1, r1);      // a has degree 4
    CHECK(e.kind == Error::PolynomialDegreeTooLarge);
  }
  ck.release(); ck2.release(); ck_small.release(); pp.release(); pp2.release();
  pc_hip_shutdown(ctx);
  printf("marlin_pst13 host mirror OK\n");
  return 0;
}
