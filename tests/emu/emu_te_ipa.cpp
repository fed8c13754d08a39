// TEST-ONLY host compilation of what the device path of InnerProductArgPC over ed_on_bls12_381 adds (te.hpp: the fold table's row
// doubling, the table fold, the out-of-place fold, the subgroup check; ipa.hpp: the functor bodies of the halving rounds instantiated for
// the curve's 252-bit scalar field), stepped lane by lane in the order abi_te.hip / field_ops_impl.hpp launch them, for comparison with
// tests/harness/te_ipa.py on a machine without a GPU.  NOT part of the product library.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/msm.hpp"
#include "../../poly_commit_amd/csrc/ipa.hpp"
#include "../../poly_commit_amd/csrc/te.hpp"

typedef pc::TeOf<pc_te_ed_on_bls12_381> TeC;
typedef pc_ed_on_bls12_381_fr FrP;
typedef pc::Fd<FrP> Fr;
typedef pc::XyzzD<TeC> Pt;
typedef pc::AffD<TeC> Aff;

template <class B> static void step(const B& body, size_t lanes) { for (size_t i = 0; i < lanes; i++) body((uint32_t)i); }

static void normalise(const uint32_t* ext, size_t count, uint32_t K, uint32_t* out) {
  std::vector<uint32_t> scratch(count * Pt::Fq::N + 1);
  pc::TeBatchAffineBody<TeC> nb{ext, scratch.data(), out, (uint32_t)count, K};
  step(nb, (count + K - 1) / K);
}

// pc_hip_te_srs_precompute_fold: tbl = rows x (n / 2) resident records of a key of n resident points
extern "C" void emu_te_ipa_fold_table(const uint32_t* key, size_t n, uint32_t rows, uint32_t K, uint32_t* tbl) {
  const size_t half = n / 2, row_words = half * Aff::WORDS;
  memcpy(tbl, key + row_words, row_words * 4);
  std::vector<uint32_t> ext(half * Pt::WORDS + 1);
  for (uint32_t b = 0; b + 1 < rows; b++) {
    pc::TeDblRowBody<TeC> d{tbl + b * row_words, ext.data()};
    step(d, half);
    normalise(ext.data(), half, K, tbl + (b + 1) * row_words);
  }
}

// pc_hip_te_ec_fold_from: out = n_half resident points; tbl may be null (the ladder).  Returns 1 if the table served the fold, 0 if the
// ladder did (no table, or a digit of u beyond `rows`).  The key is only read.
extern "C" int emu_te_ipa_fold_from(const uint32_t* key, size_t n_half, const uint32_t* tbl, uint32_t rows, const uint32_t* u_mont, uint32_t K, uint32_t* out) {
  std::vector<uint32_t> ext(n_half * Pt::WORDS + 1);
  pc::NafMasks<FrP::N> naf;
  naf.from_scalar(Fr::load(u_mont).from_mont().l);
  pc::TeTableFoldBody<TeC> t;
  int used = 0;
  if (tbl && t.dg.from_naf(naf, rows)) {
    t.key = key; t.tbl = tbl; t.half = (uint32_t)n_half; t.ext = ext.data();
    step(t, n_half);
    used = 1;
  } else {
    pc::TeEcFoldBody<TeC> f;
    f.key = key; f.half = (uint32_t)n_half; f.ext = ext.data(); f.naf = naf;
    step(f, n_half);
  }
  normalise(ext.data(), n_half, K, out);
  return used;
}

// pc_hip_te_srs_in_subgroup: one flag per point
extern "C" void emu_te_ipa_subgroup(const uint32_t* key, size_t n, uint32_t* flags) {
  pc::TeSubgroupBody<TeC> b;
  b.key = key; b.flags = flags;
  b.naf.from_scalar(FrP::MOD);
  step(b, n);
}

// the functor bodies of the rounds over the curve's scalar field, as FieldOpsImpl<FrP> launches them
extern "C" void emu_te_ipa_fr_powers(const uint32_t* z_mont, size_t n, uint32_t* out) {
  pc::FrPowersBody<FrP> body; body.out = out;
  Fr w = Fr::load(z_mont);
  for (int k = 0; k < 32; k++) { w.store(body.pt.w[k]); w = w.sqr(); }
  step(body, n);
}
extern "C" void emu_te_ipa_key_scalars(const uint32_t* c, size_t m, uint32_t* s, size_t n0, const uint32_t* fold_u, size_t fold_m, uint32_t* out_l, uint32_t* out_r) {
  if (fold_u) { pc::IpaKeyScalarUpdateBody<FrP> b{s, (uint32_t)fold_m, Fr::load(fold_u)}; step(b, n0); }
  if (out_l) { pc::IpaFixedKeyScalarsBody<FrP> b{c, s, (uint32_t)m, out_l, out_r}; step(b, n0); }
}
