// TEST-ONLY host compilation of the bodies behind MultilinearPC's setup (g2.hpp MlEqBody and ScalarMulStoreBody, ipa.hpp
// FixedBaseTableMulBody / XyzzBatchAffineBody over G1 and G2 of BLS12-381, the host table builder of host_tail.hpp), stepped lane by
// lane: validated against tests/harness/g2ref.py on a machine without a GPU.  NOT part of the product library.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/msm.hpp"
#include "../../poly_commit_amd/csrc/g2.hpp"
#include "../../poly_commit_amd/csrc/ipa.hpp"

typedef pc_curve_bls12_381 G1C;
typedef pc::G2Of<pc_curve_bls12_381> G2C;
typedef pc_bls12_381_fr FrP;

template <class B> static void step(const B& body, size_t lanes) { for (size_t i = 0; i < lanes; i++) body((uint32_t)i); }

// out[x] = prod_j e(t_j, bit_j(x)), x < 2^nv
extern "C" void emu_ml_eq(const uint32_t* t_mont, uint32_t nv, uint32_t* out) {
  pc::MlEqBody<FrP> b; b.out = out; b.set_point(t_mont, nv);
  step(b, (size_t)1 << nv);
}

// the product's table path: host window table, one table multiplication per lane, normalisation K points per lane
template <class G>
static void table_mul(const uint32_t* base, const uint32_t* scalars_mont, size_t n, uint32_t K, uint32_t* out) {
  constexpr int XW = pc::XyzzD<G>::WORDS, FW = pc::AffD<G>::WORDS / 2;
  const uint32_t Wd = pc::msm_num_windows(G::FrP::BITS, pc::FIXED_BASE_C);
  std::vector<uint32_t> tbl, res(n * XW + 1), scr(n * FW + 1);
  pc::host64::fixed_base_window_table<G>(base, pc::FIXED_BASE_C, Wd, tbl);
  pc::FixedBaseTableMulBody<G> body{scalars_mont, tbl.data(), Wd, res.data()};
  step(body, n);
  pc::XyzzBatchAffineBody<G> nb{res.data(), scr.data(), out, (uint32_t)n, K};
  step(nb, (n + K - 1) / K);
}
// the ladder path (a handful of scalars)
template <class G>
static void ladder_mul(const uint32_t* base, const uint32_t* scalars_mont, size_t n, uint32_t* out) {
  constexpr int XW = pc::XyzzD<G>::WORDS, FW = pc::AffD<G>::WORDS / 2;
  std::vector<uint32_t> res(n * XW + 1), scr(n * FW + 1);
  pc::ScalarMulStoreBody<G> body{{base, scalars_mont, 1u}, res.data()};
  step(body, n);
  pc::XyzzBatchAffineBody<G> nb{res.data(), scr.data(), out, (uint32_t)n, 1};
  step(nb, n);
}

// group 1: G1 (24-word points), 2: G2 (48-word points).  K = 0: the ladder.
extern "C" void emu_ml_fixed_base(int group, const uint32_t* base, const uint32_t* scalars_mont, size_t n, uint32_t K, uint32_t* out) {
  if (group == 1) { if (K) table_mul<G1C>(base, scalars_mont, n, K, out); else ladder_mul<G1C>(base, scalars_mont, n, out); }
  else { if (K) table_mul<G2C>(base, scalars_mont, n, K, out); else ladder_mul<G2C>(base, scalars_mont, n, out); }
}

// the upper levels: out[b] = in[2b] + in[2b + 1] for either group
extern "C" void emu_ml_pair_sums(int group, const uint32_t* in, size_t count, uint32_t K, uint32_t* out) {
  if (group == 1) {
    std::vector<uint32_t> sums(count * pc::XyzzD<G1C>::WORDS + 1), scratch(count * 12 + 1);
    pc::PairSumsBody<G1C> b{in, sums.data(), scratch.data(), out, (uint32_t)count, K};
    step(b, (count + K - 1) / K);
  } else {
    std::vector<uint32_t> sums(count * pc::XyzzD<G2C>::WORDS + 1), scratch(count * 24 + 1);
    pc::PairSumsBody<G2C> b{in, sums.data(), scratch.data(), out, (uint32_t)count, K};
    step(b, (count + K - 1) / K);
  }
}
