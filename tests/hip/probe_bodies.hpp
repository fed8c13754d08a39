// TEST-ONLY probe bodies: ONE primitive of csrc/ (fp32.hpp, fp30.hpp, fp2.hpp, ec.hpp) per lane, raw words in, raw words out, so
// that tests/test_device_primitives_{gpu,cpu}.py can hand the device's own multiplier the boundary operands of every class and
// compare the result bit for bit with Python integers and with the host compilation of the same body.
//
// A body is written like the product's kernel bodies: a PC_HD functor over plain word arrays, operator()(lane).  Every body has the
// members {in, out, aux, param}; lane i reads in + i * IN_WORDS and writes out + i * OUT_WORDS.  Inputs are in-contract for the
// function they are given to (the tests build them per operand class); nothing here checks them.
#pragma once
#include "../../poly_commit_amd/csrc/ec.hpp"

namespace probe {
using namespace pc;

// ---- Fd<P>: four operands a, b, c, d of N words, one result of N words -----------------------------------------------------------
enum FieldOp {
  F_MUL = 0, F_SQR, F_MUL_ADD_MUL, F_FROM_MONT, F_TO_MONT, F_ADD, F_SUB, F_DBL, F_NEG, F_INV,
  // LAZY_OK only; raw outputs
  F_MUL_LZ, F_SQR_LZ, F_MUL_ADD_MUL_LZ, F_SUB_LZ, F_DBL_LZ, F_NEG_LZ, F_NEG_LZ_CANONICAL, F_IS_ZERO_LZ, F_CANON1, F_CANON,
  F_NOPS
};
template <class P>
struct FieldBodies {
  template <int OP>
  struct Body {
    typedef Fd<P> F;
    static constexpr int N = F::N, IN_WORDS = 4 * N, OUT_WORDS = N;
    static constexpr bool SUPPORTED = OP < F_MUL_LZ || F::LAZY_OK;
    const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
    PC_HD void operator()(uint32_t lane) const {
      const uint32_t* p = in + (size_t)lane * IN_WORDS;
      const F a = F::load(p), b = F::load(p + N), c = F::load(p + 2 * N), d = F::load(p + 3 * N);
      F r = F::zero();
      if constexpr (OP == F_MUL) r = a.mul(b);
      else if constexpr (OP == F_SQR) r = a.sqr();
      else if constexpr (OP == F_MUL_ADD_MUL) r = a.mul_add_mul(b, c, d);
      else if constexpr (OP == F_FROM_MONT) r = a.from_mont();
      else if constexpr (OP == F_TO_MONT) r = a.to_mont();
      else if constexpr (OP == F_ADD) r = a.add(b);
      else if constexpr (OP == F_SUB) r = a.sub(b);
      else if constexpr (OP == F_DBL) r = a.dbl();
      else if constexpr (OP == F_NEG) r = a.neg();
      else if constexpr (OP == F_INV) r = a.inv();
      else if constexpr (OP == F_MUL_LZ) r = a.mul_lz(b);
      else if constexpr (OP == F_SQR_LZ) r = a.sqr_lz();
      else if constexpr (OP == F_MUL_ADD_MUL_LZ) r = a.mul_add_mul_lz(b, c, d);
      else if constexpr (OP == F_SUB_LZ) r = a.sub_lz(b);
      else if constexpr (OP == F_DBL_LZ) r = a.dbl_lz();
      else if constexpr (OP == F_NEG_LZ) r = a.neg_lz();
      else if constexpr (OP == F_NEG_LZ_CANONICAL) r = a.neg_lz_canonical();
      else if constexpr (OP == F_IS_ZERO_LZ) r.l[0] = a.is_zero_lz() ? 1u : 0u;
      else if constexpr (OP == F_CANON1) r = a.canon1();
      else if constexpr (OP == F_CANON) r = a.canon();
      r.store(out + (size_t)lane * OUT_WORDS);
    }
  };
};

// ---- Fq30: four operands of 13 limbs, one result of 13 limbs; every instantiation XyzzR30::add_affine makes ----------------------
enum Fq30Op {
  Q_MUL_64_2 = 0, Q_MUL_66_8, Q_MUL_64_8, Q_MUL_2_8, Q_MUL_2_2, Q_REDUCE, Q_SQR_66, Q_MUL_ADD_MUL_66_16_64_2,
  Q_SUB_64, Q_SUB_2, Q_SUB_14, Q_SUB_DBL_4, Q_NEG_64, Q_FROM32, Q_TO32, Q_IS_ZERO_MODP_66, Q_IS_ZERO_EXACT, Q_ONE,
  Q_NOPS
};
template <int OP>
struct Fq30Body {
  static constexpr int W = 13, IN_WORDS = 4 * W, OUT_WORDS = W;
  static constexpr bool SUPPORTED = true;
  const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
  static PC_HD Fq30 ld(const uint32_t* p) { Fq30 r; PC_UNROLL for (int i = 0; i < W; i++) r.l[i] = p[i]; return r; }
  PC_HD void operator()(uint32_t lane) const {
    const uint32_t* p = in + (size_t)lane * IN_WORDS;
    const Fq30 a = ld(p), b = ld(p + W), c = ld(p + 2 * W), d = ld(p + 3 * W);
    Fq30 r = Fq30::zero();
    if constexpr (OP == Q_MUL_64_2) r = Fq30::mul<64, 2>(a, b);
    else if constexpr (OP == Q_MUL_66_8) r = Fq30::mul<66, 8>(a, b);
    else if constexpr (OP == Q_MUL_64_8) r = Fq30::mul<64, 8>(a, b);
    else if constexpr (OP == Q_MUL_2_8) r = Fq30::mul<2, 8>(a, b);
    else if constexpr (OP == Q_MUL_2_2) r = Fq30::mul<2, 2>(a, b);
    else if constexpr (OP == Q_REDUCE) r = a.reduce();
    else if constexpr (OP == Q_SQR_66) r = Fq30::sqr<66>(a);
    else if constexpr (OP == Q_MUL_ADD_MUL_66_16_64_2) r = Fq30::mul_add_mul<66, 16, 64, 2>(a, b, c, d);
    else if constexpr (OP == Q_SUB_64) r = Fq30::sub<64>(a, b);
    else if constexpr (OP == Q_SUB_2) r = Fq30::sub<2>(a, b);
    else if constexpr (OP == Q_SUB_14) r = Fq30::sub<14>(a, b);
    else if constexpr (OP == Q_SUB_DBL_4) r = Fq30::sub_dbl<4>(a, b);
    else if constexpr (OP == Q_NEG_64) r = Fq30::neg<64>(a);
    else if constexpr (OP == Q_FROM32) r = Fq30::from32(Fq30::F32::load(p));
    else if constexpr (OP == Q_TO32) { const Fq30::F32 w = a.to32(); PC_UNROLL for (int i = 0; i < 12; i++) r.l[i] = w.l[i]; }
    else if constexpr (OP == Q_IS_ZERO_MODP_66) r.l[0] = a.is_zero_modp<66>() ? 1u : 0u;
    else if constexpr (OP == Q_IS_ZERO_EXACT) r.l[0] = a.is_zero_exact() ? 1u : 0u;
    else if constexpr (OP == Q_ONE) r = Fq30::one();
    uint32_t* o = out + (size_t)lane * OUT_WORDS;
    PC_UNROLL for (int i = 0; i < W; i++) o[i] = r.l[i];
  }
};

// ---- Fq2D<BLS12-381 Fq>: four operands of 24 words, one result -------------------------------------------------------------------
enum Fq2Op { E_MUL = 0, E_SQR, E_MUL_ADD_MUL, E_INV, E_ADD, E_SUB, E_NEG, E_NOPS };
template <int OP>
struct Fq2Body {
  typedef Fq2D<pc_bls12_381_fq> F;
  static constexpr int N = F::N, IN_WORDS = 4 * N, OUT_WORDS = N;
  static constexpr bool SUPPORTED = true;
  const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
  PC_HD void operator()(uint32_t lane) const {
    const uint32_t* p = in + (size_t)lane * IN_WORDS;
    const F a = F::load(p), b = F::load(p + N), c = F::load(p + 2 * N), d = F::load(p + 3 * N);
    F r = F::zero();
    if constexpr (OP == E_MUL) r = a.mul(b);
    else if constexpr (OP == E_SQR) r = a.sqr();
    else if constexpr (OP == E_MUL_ADD_MUL) r = a.mul_add_mul(b, c, d);
    else if constexpr (OP == E_INV) r = a.inv();
    else if constexpr (OP == E_ADD) r = a.add(b);
    else if constexpr (OP == E_SUB) r = a.sub(b);
    else if constexpr (OP == E_NEG) r = a.neg();
    r.store(out + (size_t)lane * OUT_WORDS);
  }
};

// ---- XyzzD<C>: in = P (XYZZ, 4 FN words) | Q (XYZZ; an affine operand is its first 2 FN words) | flag; out = the raw XYZZ words of
// the result | its affine point (the lazy addition: of canonical()) ------------------------------------------------------------------
enum CurveOp { C_ADD_AFFINE = 0, C_ADD_AFFINE_LZ, C_ADD, C_DBL, C_DBL_AFFINE, C_TO_AFFINE, C_NOPS };
template <class C>
struct CurveBodies {
  template <int OP>
  struct Body {
    typedef XyzzD<C> Pt; typedef AffD<C> Aff; typedef typename Pt::Fq Fq;
    static constexpr int FN = Fq::N, IN_WORDS = 8 * FN + 1, OUT_WORDS = 6 * FN;
    static constexpr bool SUPPORTED = OP != C_ADD_AFFINE_LZ || Fq::LAZY_OK;
    const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
    PC_HD void operator()(uint32_t lane) const {
      const uint32_t* p = in + (size_t)lane * IN_WORDS;
      Pt r = Pt::load(p);
      const bool flag = p[8 * FN] != 0;
      Aff a;
      if constexpr (OP == C_ADD_AFFINE) { r.add_affine(Aff::load(p + 4 * FN)); a = r.to_affine(); }
      else if constexpr (OP == C_ADD_AFFINE_LZ) { r.add_affine_lz(Aff::load(p + 4 * FN), flag); a = r.canonical().to_affine(); }
      else if constexpr (OP == C_ADD) { r.add(Pt::load(p + 4 * FN)); a = r.to_affine(); }
      else if constexpr (OP == C_DBL) { r = r.dbl(); a = r.to_affine(); }
      else if constexpr (OP == C_DBL_AFFINE) { r = Pt::dbl_affine(Aff::load(p + 4 * FN)); a = r.to_affine(); }
      else { a = r.to_affine(); }
      uint32_t* o = out + (size_t)lane * OUT_WORDS;
      r.store(o); a.store(o + 4 * FN);
    }
  };
};

// ---- the running sum in radix 2^30 against the lazily reduced and the canonical one: the device form of tests/emu/emu_fq30.cpp's chain.
// One lane per index list: in = count | idx[param] (idx = table entry | sign << 31); aux = 64 affine points, entry 0 infinite.
// out = bad steps | hash of the to32() words of every step | to32() raw | to32().canonical() | lazy sum, canonical | canonical sum
struct Chain30Body {
  typedef pc_curve_bls12_381 C; typedef XyzzD<C> Pt; typedef AffD<C> Aff;
  static constexpr int OUT_WORDS = 2 + 4 * 48;
  const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
  // limbs 0..11 below 2^30 and value <= V p
  template <int V>
  static PC_HD bool in_class(const Fq30& a) {
    constexpr Fq30::L13 k = Fq30::kp(V);
    uint32_t high = 0;
    PC_UNROLL for (int i = 0; i < 12; i++) high |= a.l[i] >> 30;
    if (high) return false;
    for (int i = 12; i >= 0; i--) { if (a.l[i] < k.v[i]) return true; if (a.l[i] > k.v[i]) return false; }
    return true;
  }
  static PC_HD bool same(const Pt& x, const Pt& y) { return x.X.eq(y.X) && x.Y.eq(y.Y) && x.ZZ.eq(y.ZZ) && x.ZZZ.eq(y.ZZZ); }
  PC_HD void operator()(uint32_t lane) const {
    const uint32_t* p = in + (size_t)lane * (1 + param);
    const uint32_t n = p[0] < param ? p[0] : param;
    XyzzR30 a30 = XyzzR30::infinity();
    Pt alz = Pt::infinity(), ac = Pt::infinity();
    uint32_t bad = 0, hash = 0x811c9dc5u;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t e = p[1 + i];
      const Aff pt = Aff::load(aux + (size_t)(e & 63u) * Aff::WORDS);
      const bool neg = (e >> 31) != 0;
      a30.add_affine(pt, neg);
      alz.add_affine_lz(pt, neg);
      ac.add_affine(pt.neg_if(neg));
      bool ok = in_class<64>(a30.X) && in_class<64>(a30.Y) && in_class<2>(a30.ZZ) && in_class<2>(a30.ZZZ);
      const Pt raw = a30.to32(), c30 = raw.canonical(), clz = alz.canonical();
      uint32_t w[Pt::WORDS]; raw.store(w);
      for (int k = 0; k < Pt::WORDS; k++) hash = (hash ^ w[k]) * 0x01000193u;
      ok = ok && (c30.is_inf() ? clz.is_inf() : same(c30, clz)) && c30.is_inf() == a30.is_inf();
      bad += ok ? 0u : 1u;
    }
    uint32_t* o = out + (size_t)lane * OUT_WORDS;
    o[0] = bad; o[1] = hash;
    const Pt raw = a30.to32();
    raw.store(o + 2); raw.canonical().store(o + 2 + 48); alz.canonical().store(o + 2 + 96); ac.store(o + 2 + 144);
  }
};

}  // namespace probe
