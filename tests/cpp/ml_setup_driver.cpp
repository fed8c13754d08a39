// Test driver: MultilinearPC setup / trim (from resident parameters) / commit / open of the C++ host mirror
// (poly_commit_amd/host/multilinear_pc.hpp) on inputs read from a file -- tests/test_ml_setup_gpu.py compares the output with
// tests/harness/g2ref.py.
//   file in : u32 nv | u32 supported | g 96 B | h 192 B | t nv Fr | evals 2^supported Fr | point supported Fr
//   file out: g_mask nv x 96 B | commitment 96 B | supported proofs x 192 B
#include <stdio.h>
#include <stdlib.h>
#include "../../poly_commit_amd/host/multilinear_pc.hpp"
using namespace pc_host;

int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: ml_setup_driver in out\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { printf("cannot open %s\n", argv[1]); return 2; }
  auto rd = [&](void* p, size_t b) { if (fread(p, 1, b, in) != b) { printf("short input\n"); exit(2); } };
  uint32_t nv = 0, sup = 0; rd(&nv, 4); rd(&sup, 4);
  if (nv < 1 || nv > 24 || sup < 1 || sup > nv) { printf("bad nv\n"); return 2; }
  uint64_t gxy[12], hw[24]; rd(gxy, sizeof gxy); rd(hw, sizeof hw);
  std::vector<FrT<Bls12_381>> t(nv), evals((size_t)1 << sup), point(sup);
  rd(t.data(), nv * 32); rd(evals.data(), evals.size() * 32); rd(point.data(), sup * 32);
  fclose(in);
  pc_ctx* ctx = nullptr;
  int rc = pc_hip_init(0, &ctx);
  if (rc != PC_OK) { printf("pc_hip_init failed: %s\n", pc_hip_strerror(rc)); return rc == PC_ERR_NO_DEVICE ? 77 : 1; }
  MlResidentParams pp;
  MlCommitterKey ck;
  int r = 1;
  do {
    const G1Affine<Bls12_381> g = G1Affine<Bls12_381>::from_xy(gxy, false);
    if (Error e = MultilinearPC::setup(ctx, nv, g, G2AffineBls::from_words(hw), t, pp)) { printf("setup: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    if (pc_hip_srs_len(pp.powers_of_g) != ((size_t)2 << nv) - 2 || pc_hip_g2_srs_len(pp.powers_of_h) != ((size_t)2 << nv) - 1) { printf("key sizes\n"); break; }
    if (MultilinearPC::trim(ctx, pp, nv + 1, ck).kind != Error::InvalidNumberOfVariables) { printf("supported > nv not reported as InvalidNumberOfVariables\n"); break; }
    if (Error e = MultilinearPC::trim(ctx, pp, sup, ck)) { printf("trim: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    G1Affine<Bls12_381> comm = G1Affine<Bls12_381>::zero();
    if (Error e = MultilinearPC::commit(ctx, ck, evals, comm)) { printf("commit: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    MlProof proof;
    if (Error e = MultilinearPC::open(ctx, ck, evals, point, proof)) { printf("open: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    FILE* out = fopen(argv[2], "wb");
    uint64_t xy[12];
    for (auto& m : pp.g_mask) { m.to_xy(xy); fwrite(xy, 1, sizeof xy, out); }
    comm.to_xy(xy); fwrite(xy, 1, sizeof xy, out);
    for (auto& p : proof.proofs) { uint64_t w[24]; p.to_words(w); fwrite(w, 1, sizeof w, out); }
    fclose(out);
    printf("multilinear_pc setup/trim/commit/open OK (nv %u, supported %u)\n", nv, sup);
    r = 0;
  } while (0);
  ck.release();
  pp.release();
  pc_hip_shutdown(ctx);
  return r;
}
