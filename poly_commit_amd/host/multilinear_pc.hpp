// C++ host mirror of MultilinearPC's setup / trim / commit / open (poly-commit/src/multilinear_pc/mod.rs, the XZZPD19 multilinear KZG
// scheme), above the C ABI:
//
//   setup    multilinear_pc/mod.rs:28-86     the eq tables of the trapdoor, g.batch_mul and h.batch_mul, on the device: both
//                                            parameter lists stay resident (MlResidentParams)                -> pc_hip_ml_setup
//   trim     multilinear_pc/mod.rs:91-111    powers_of_g[0] becomes a resident pc_srs, every powers_of_h[i] is uploaded and
//                                            reduced to its pair sums on the device                         -> pc_hip_srs_upload,
//                                                                                                              pc_hip_g2_srs_upload, pc_hip_g2_srs_pair_sums
//   commit   multilinear_pc/mod.rs:114-128   one G1 MSM of the evaluations over powers_of_g[0]              -> pc_hip_msm
//   open     multilinear_pc/mod.rs:131-168   nv rounds: halve the table, one G2 MSM                         -> pc_hip_ml_open
//
// The reference's open multiplies BOTH points of a pair by the same scalar (scalars[x] = q[x >> 1], :158-160), so the resident key
// of round i is the list of H[2b] + H[2b + 1]: the same group elements, half the additions, the same proofs bit for bit.
// trim has two forms: from host parameters (every level of powers_of_h crosses to the device), and from the resident parameters of
// setup (device to device: the pair sums of a level are the next level, so the key of open is a suffix of powers_of_h).
// BLS12-381 only (the curve the reference instantiates, :247).  setup takes the trapdoor from the caller (the reference samples it,
// :34); check (:172-200, pairings) stays with the caller.
#pragma once
#include "kzg10.hpp"

namespace pc_host {

// G2 affine point as arkworks holds it: x.c0, x.c1, y.c0, y.c1 (Montgomery), and the flag
struct G2AffineBls {
  uint64_t w[24];
  bool infinity = true;
  static G2AffineBls zero() { G2AffineBls a; memset(a.w, 0, sizeof(a.w)); a.infinity = true; return a; }
  static G2AffineBls from_words(const uint64_t* in) {
    G2AffineBls a; memcpy(a.w, in, sizeof(a.w));
    bool inf = true; for (int i = 0; i < 24; i++) inf &= in[i] == 0;
    a.infinity = inf; return a;
  }
  void to_words(uint64_t* out) const { if (infinity) memset(out, 0, sizeof(w)); else memcpy(out, w, sizeof(w)); }
};

struct MlUniversalParams {                           // data_structures.rs: UniversalParams { num_vars, powers_of_g, powers_of_h, .. }
  size_t num_vars = 0;
  std::vector<std::vector<G1Affine<Bls12_381>>> powers_of_g;      // level i: 2^(num_vars - i) points
  std::vector<std::vector<G2AffineBls>> powers_of_h;
};

struct MlResidentParams {                            // UniversalParams made and kept on the device (pc_hip_ml_setup)
  size_t num_vars = 0;
  pc_srs* powers_of_g = nullptr;                     // 2^(nv+1) - 2 points, level i at 2^(nv+1) - 2^(nv-i+1)
  pc_g2_srs* powers_of_h = nullptr;                  // the same levels and h appended: 2^(nv+1) - 1 points
  G1Affine<Bls12_381> g = G1Affine<Bls12_381>::zero();
  G2AffineBls h = G2AffineBls::zero();
  std::vector<G1Affine<Bls12_381>> g_mask;           // g_mask[i] = t_i * g
  size_t level_offset(size_t i) const { return ((size_t)2 << num_vars) - ((size_t)2 << (num_vars - i)); }
  void release() { if (powers_of_g) pc_hip_srs_free(powers_of_g); if (powers_of_h) pc_hip_g2_srs_free(powers_of_h); powers_of_g = nullptr; powers_of_h = nullptr; }
};

struct MlCommitterKey {                              // CommitterKey { nv, powers_of_g, powers_of_h, .. }: resident form
  size_t nv = 0;
  pc_srs* powers_of_g0 = nullptr;                    // powers_of_g[0], 2^nv points
  pc_g2_srs* pair_key = nullptr;                     // pair sums of powers_of_h[0 .. nv): 2^nv - 1 points, round i at 2^nv - 2^(nv - i)
  void release() { if (powers_of_g0) pc_hip_srs_free(powers_of_g0); if (pair_key) pc_hip_g2_srs_free(pair_key); powers_of_g0 = nullptr; pair_key = nullptr; }
};

struct MlProof { std::vector<G2AffineBls> proofs; };      // Proof { proofs }

struct MultilinearPC {
  typedef Bls12_381 E;
  typedef FrT<E> Fr;
  static Error backend_error(pc_ctx* ctx, int rc) {
    Error e; e.kind = Error::Backend; e.msg = std::string(pc_hip_strerror(rc)) + ": " + pc_hip_last_error(ctx); return e;
  }
  // setup (mod.rs:28-86) with the trapdoor t given: nothing but g, h and t crosses to the device
  static Error setup(pc_ctx* ctx, size_t num_vars, const G1Affine<E>& g, const G2AffineBls& h, const std::vector<Fr>& t, MlResidentParams& pp) {
    if (num_vars < 1 || t.size() != num_vars) { Error e; e.kind = Error::InvalidNumberOfVariables; e.a = num_vars; return e; }
    pp.release(); pp.num_vars = num_vars; pp.g = g; pp.h = h;
    uint64_t gxy[12], hw[24];
    g.to_xy(gxy); h.to_words(hw);
    std::vector<uint64_t> mask(num_vars * 12);
    const int rc = pc_hip_ml_setup(ctx, E::ID, (unsigned)num_vars, gxy, hw, t.data(), &pp.powers_of_g, &pp.powers_of_h, mask.data());
    if (rc != PC_OK) return backend_error(ctx, rc);
    pp.g_mask.clear();
    for (size_t i = 0; i < num_vars; i++) {
      bool inf = true; for (int k = 0; k < 12; k++) inf &= mask[i * 12 + k] == 0;
      pp.g_mask.push_back(G1Affine<E>::from_xy(&mask[i * 12], inf));
    }
    return Error();
  }
  // trim (mod.rs:91-111) from resident parameters: two device-to-device copies
  static Error trim(pc_ctx* ctx, const MlResidentParams& pp, size_t supported_num_vars, MlCommitterKey& ck) {
    if (supported_num_vars < 1 || supported_num_vars > pp.num_vars) { Error e; e.kind = Error::InvalidNumberOfVariables; e.a = supported_num_vars; return e; }
    ck.release(); ck.nv = supported_num_vars;
    const int rc = pc_hip_ml_trim(ctx, pp.powers_of_g, pp.powers_of_h, (unsigned)pp.num_vars, (unsigned)supported_num_vars, &ck.powers_of_g0, &ck.pair_key);
    if (rc != PC_OK) return backend_error(ctx, rc);
    return Error();
  }
  // trim (mod.rs:91-111): the levels [to_reduce, num_vars) of the universal parameters, made resident
  static Error trim(pc_ctx* ctx, const MlUniversalParams& pp, size_t supported_num_vars, MlCommitterKey& ck) {
    if (supported_num_vars < 1 || supported_num_vars > pp.num_vars) { Error e; e.kind = Error::InvalidNumberOfVariables; e.a = supported_num_vars; return e; }
    const size_t to_reduce = pp.num_vars - supported_num_vars, nv = supported_num_vars, n = (size_t)1 << nv;
    ck.release(); ck.nv = nv;
    std::vector<uint64_t> buf(n * 12);
    for (size_t i = 0; i < n; i++) pp.powers_of_g[to_reduce][i].to_xy(&buf[i * 12]);
    int rc = pc_hip_srs_upload(ctx, E::ID, buf.data(), n, 0, PC_MEM_HOST, &ck.powers_of_g0);
    if (rc != PC_OK) return backend_error(ctx, rc);
    std::vector<uint64_t> zeros((n - 1) * 24, 0);
    rc = pc_hip_g2_srs_upload(ctx, E::ID, zeros.data(), n - 1, 0, PC_MEM_HOST, &ck.pair_key);
    if (rc != PC_OK) { ck.release(); return backend_error(ctx, rc); }
    for (size_t i = 0; i < nv; i++) {
      const std::vector<G2AffineBls>& lvl = pp.powers_of_h[to_reduce + i];
      const size_t m = n >> i;
      std::vector<uint64_t> hb(m * 24);
      for (size_t x = 0; x < m; x++) lvl[x].to_words(&hb[x * 24]);
      pc_g2_srs* level = nullptr;
      rc = pc_hip_g2_srs_upload(ctx, E::ID, hb.data(), m, 0, PC_MEM_HOST, &level);
      if (rc == PC_OK) rc = pc_hip_g2_srs_pair_sums(ctx, level, 0, m / 2, ck.pair_key, n - m);
      pc_hip_g2_srs_free(level);
      if (rc != PC_OK) { ck.release(); return backend_error(ctx, rc); }
    }
    return Error();
  }
  // commit (mod.rs:114-128): msm_bigint(powers_of_g[0], evaluations)
  static Error commit(pc_ctx* ctx, const MlCommitterKey& ck, const std::vector<Fr>& evals, G1Affine<E>& out) {
    if (evals.size() != (size_t)1 << ck.nv) { Error e; e.kind = Error::InvalidNumberOfVariables; e.a = evals.size(); return e; }
    uint64_t xy[12]; int inf = 0;
    const int rc = pc_hip_msm(ctx, ck.powers_of_g0, 0, evals.data(), PC_SCALARS_MONTGOMERY, PC_MEM_HOST, evals.size(), xy, &inf);
    if (rc != PC_OK) return backend_error(ctx, rc);
    out = G1Affine<E>::from_xy(xy, inf != 0);
    return Error();
  }
  // open (mod.rs:131-168)
  static Error open(pc_ctx* ctx, const MlCommitterKey& ck, const std::vector<Fr>& evals, const std::vector<Fr>& point, MlProof& proof) {
    if (evals.size() != (size_t)1 << ck.nv || point.size() != ck.nv) { Error e; e.kind = Error::InvalidNumberOfVariables; e.a = point.size(); return e; }
    std::vector<uint64_t> out(ck.nv * 24);
    const int rc = pc_hip_ml_open(ctx, ck.pair_key, evals.data(), PC_MEM_HOST, (unsigned)ck.nv, point.data(), out.data(), nullptr);
    if (rc != PC_OK) return backend_error(ctx, rc);
    proof.proofs.clear();
    for (size_t i = 0; i < ck.nv; i++) proof.proofs.push_back(G2AffineBls::from_words(&out[i * 24]));
    return Error();
  }
};

}  // namespace pc_host
