// TEST-ONLY host compilation of the MarlinPST13 kernels (csrc/pst13.hpp): the bodies of the monomial evaluations, the scatter's two
// passes, the division along every variable and the re-ranking of trim, every lane stepped on the host with the binomial table in
// host memory -- the index arithmetic (unrank, the slot walk of a fiber) is exactly what the kernels run.  Validated against
// tests/harness/pst13.py on a machine without a GPU.  NOT part of the product library.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/pst13.hpp"

struct CpuStepBackend {};

extern "C" uint32_t emu_pst13_table_entry(uint32_t n, uint32_t d, uint32_t v, uint32_t r) { return pc::pst13_table(n, d)[(size_t)v * (d + 1) + r]; }

// unrank of the layout (nv, budget) read from the table of (n, d), as a pass of the division and trim do
extern "C" uint32_t emu_pst13_unrank(uint32_t n, uint32_t d, uint32_t nv, uint32_t budget, uint32_t rank, uint8_t* out_exps) {
  const std::vector<uint32_t> T = pc::pst13_table(n, d);
  pc::Pst13Exps e; e.clear();
  const uint32_t deg = pc::pst13_unrank(T.data(), d + 1, rank, 0, nv, budget, e);
  for (uint32_t j = 0; j < nv; j++) out_exps[j] = (uint8_t)e.get(j);
  return deg;
}
extern "C" uint32_t emu_pst13_rank(uint32_t n, uint32_t d, uint32_t nv, uint32_t budget, const uint8_t* exps) {
  const std::vector<uint32_t> T = pc::pst13_table(n, d);
  pc::Pst13Exps e;
  pc::pst13_load_exps(exps, nv, e);
  return pc::pst13_rank(T.data(), d + 1, e, 0, nv, budget);
}

template <class FrP>
static void divide(uint32_t n, uint32_t d, const uint32_t* p, const uint32_t* z, uint32_t* quot, const uint64_t* offs, uint32_t* value) {
  CpuStepBackend be;
  const std::vector<uint32_t> T = pc::pst13_table(n, d);
  const size_t fibers = T[(size_t)(n - 1) * (d + 1) + d];
  std::vector<uint32_t> ping(fibers * FrP::N + FrP::N, 0xA5A5A5A5u), pong(fibers * FrP::N + FrP::N, 0xA5A5A5A5u);
  const uint32_t* last = pc::pst13_divide<FrP>(be, T.data(), T.data(), n, d, p, z, quot, offs, ping.data(), pong.data());
  memcpy(value, last, (size_t)FrP::N * 4);
  for (uint32_t w = 0; w < FrP::N; w++) if (ping[fibers * FrP::N + w] != 0xA5A5A5A5u || pong[fibers * FrP::N + w] != 0xA5A5A5A5u) abort();
}
// the n passes (n >= 2): quotient i at quot + offs[i] elements, value = p(z)
extern "C" void emu_pst13_divide(int curve, uint32_t n, uint32_t d, const uint32_t* p, const uint32_t* z, uint32_t* quot, const uint64_t* offs, uint32_t* value) {
  if (curve == 0) divide<pc_bls12_381_fr>(n, d, p, z, quot, offs, value); else divide<pc_bn254_fr>(n, d, p, z, quot, offs, value);
}

template <class FrP>
static uint32_t scatter(uint32_t n, uint32_t d, const uint8_t* exps, const uint32_t* coeffs, uint32_t terms, uint32_t* out) {
  CpuStepBackend be;
  const std::vector<uint32_t> T = pc::pst13_table(n, d);
  const size_t M = T[(size_t)n * (d + 1) + d];
  std::vector<uint32_t> owner(M, 0);
  uint32_t flags = 0;
  memset(out, 0, M * FrP::N * 4);
  pc::Pst13ClaimBody claim{exps, owner.data(), &flags, n, d};
  pc::pst13_launch(be, claim, terms, T.data(), (uint32_t)T.size());
  pc::Pst13WriteBody<FrP> write{exps, coeffs, owner.data(), &flags, out, n, d};
  pc::pst13_launch(be, write, terms, T.data(), (uint32_t)T.size());
  return flags;
}
// returns the flags: 1 = a term of degree above d, 2 = a repeated tuple
extern "C" uint32_t emu_pst13_scatter(int curve, uint32_t n, uint32_t d, const uint8_t* exps, const uint32_t* coeffs, uint32_t terms, uint32_t* out) {
  return curve == 0 ? scatter<pc_bls12_381_fr>(n, d, exps, coeffs, terms, out) : scatter<pc_bn254_fr>(n, d, exps, coeffs, terms, out);
}

template <class FrP>
static void monomials(uint32_t n, uint32_t d, const uint32_t* pw, uint32_t* out) {
  CpuStepBackend be;
  const std::vector<uint32_t> T = pc::pst13_table(n, d);
  pc::Pst13MonomialBody<FrP> b{pw, out, n, d};
  pc::pst13_launch(be, b, T[(size_t)n * (d + 1) + d], T.data(), (uint32_t)T.size());
}
// pw: n x (d + 1) powers
extern "C" void emu_pst13_monomials(int curve, uint32_t n, uint32_t d, const uint32_t* pw, uint32_t* out) {
  if (curve == 0) monomials<pc_bls12_381_fr>(n, d, pw, out); else monomials<pc_bn254_fr>(n, d, pw, out);
}

// trim's gather on `aw`-word records
extern "C" void emu_pst13_rerank(uint32_t n, uint32_t d, uint32_t s, uint32_t aw, const uint32_t* in, uint32_t* out) {
  CpuStepBackend be;
  const std::vector<uint32_t> T = pc::pst13_table(n, d);
  pc::Pst13RerankBody b{in, out, n, d, s, aw};
  pc::pst13_launch(be, b, T[(size_t)n * (d + 1) + s], T.data(), (uint32_t)T.size());
}
