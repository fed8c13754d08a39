// Test driver: MultilinearPC trim / commit / open of the C++ host mirror (poly_commit_amd/host/multilinear_pc.hpp) on inputs read from a
// file; commitment and proofs written to a file -- tests/test_multilinear_pc_gpu.py compares them with tests/harness/g2ref.py.
//   file in : u32 nv | powers_of_g[0] 2^nv x 96 B | powers_of_h[i] 2^(nv-i) x 192 B for i < nv | evals 2^nv Fr | point nv Fr
//   file out: commitment 96 B | nv proofs x 192 B
#include <stdio.h>
#include <stdlib.h>
#include "../../poly_commit_amd/host/multilinear_pc.hpp"
using namespace pc_host;

int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: multilinear_pc_driver in out\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { printf("cannot open %s\n", argv[1]); return 2; }
  auto rd = [&](void* p, size_t b) { if (fread(p, 1, b, in) != b) { printf("short input\n"); exit(2); } };
  uint32_t nv = 0; rd(&nv, 4);
  if (nv < 1 || nv > 24) { printf("bad nv\n"); return 2; }
  const size_t n = (size_t)1 << nv;
  MlUniversalParams pp; pp.num_vars = nv;
  pp.powers_of_g.resize(nv); pp.powers_of_h.resize(nv);
  for (size_t i = 0; i < n; i++) {
    uint64_t xy[12]; rd(xy, sizeof xy);
    bool inf = true; for (int k = 0; k < 12; k++) inf &= xy[k] == 0;
    pp.powers_of_g[0].push_back(G1Affine<Bls12_381>::from_xy(xy, inf));
  }
  for (uint32_t i = 0; i < nv; i++)
    for (size_t x = 0; x < (n >> i); x++) { uint64_t w[24]; rd(w, sizeof w); pp.powers_of_h[i].push_back(G2AffineBls::from_words(w)); }
  std::vector<FrT<Bls12_381>> evals(n), point(nv);
  rd(evals.data(), n * 32); rd(point.data(), nv * 32);
  fclose(in);
  pc_ctx* ctx = nullptr;
  int rc = pc_hip_init(0, &ctx);
  if (rc != PC_OK) { printf("pc_hip_init failed: %s\n", pc_hip_strerror(rc)); return rc == PC_ERR_NO_DEVICE ? 77 : 1; }
  MlCommitterKey ck;
  int r = 1;
  do {
    if (Error e = MultilinearPC::trim(ctx, pp, nv, ck)) { printf("trim: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    G1Affine<Bls12_381> comm = G1Affine<Bls12_381>::zero();
    if (Error e = MultilinearPC::commit(ctx, ck, evals, comm)) { printf("commit: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    MlProof proof;
    if (Error e = MultilinearPC::open(ctx, ck, evals, point, proof)) { printf("open: kind %d %s\n", (int)e.kind, e.msg.c_str()); break; }
    { std::vector<FrT<Bls12_381>> shorter(point.begin(), point.end() - 1); MlProof p2;
      if (MultilinearPC::open(ctx, ck, evals, shorter, p2).kind != Error::InvalidNumberOfVariables) { printf("short point not reported as InvalidNumberOfVariables\n"); break; } }
    FILE* out = fopen(argv[2], "wb");
    uint64_t xy[12]; comm.to_xy(xy); fwrite(xy, 1, sizeof xy, out);
    for (auto& p : proof.proofs) { uint64_t w[24]; p.to_words(w); fwrite(w, 1, sizeof w, out); }
    fclose(out);
    printf("multilinear_pc trim/commit/open OK (nv %u)\n", nv);
    r = 0;
  } while (0);
  ck.release();
  pc_hip_shutdown(ctx);
  return r;
}
