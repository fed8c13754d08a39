// TEST-ONLY probe bodies of the twisted Edwards code (csrc/te.hpp): ONE primitive of XyzzD<TeOf<T>> / AffD<TeOf<T>> per lane, and the
// chain of mixed additions on a running sum, for tests/test_te_primitives_{gpu,cpu}.py (tests/harness/teprobe.py).  Written like
// probe_bodies.hpp: PC_HD functors over plain word arrays with the members {in, out, aux, param}; inputs are in-contract for the
// function they are given to, nothing here checks them.  The product's own kernel bodies (TeEcFoldBody, ...) are run as they are by
// the adapters of probe_te.hip.
#pragma once
#include "../../poly_commit_amd/csrc/te.hpp"

namespace probe {
using namespace pc;

// in = P (X | Y | Z | T, 4 FN words) | Q (the same; an affine operand is its first AffD::WORDS words, the resident x | y | td, or the
// caller's x | y for T_DERIVE); out = the raw X | Y | Z | T of the result | to_affine() of it in resident words.  The operations whose
// result is an affine record (T_DERIVE, T_NEG) leave the raw words zero and store the record as it is.
enum TeOp { T_MADD = 0, T_ADD, T_DBL, T_TO_AFFINE, T_FROM_AFFINE, T_DERIVE, T_NEG, T_NOPS };
template <class G>
struct TeBodies {
  template <int OP>
  struct Body {
    typedef XyzzD<G> Pt; typedef AffD<G> Aff;
    static constexpr int FN = Pt::Fq::N, IN_WORDS = 8 * FN, OUT_WORDS = 4 * FN + Aff::WORDS;
    static constexpr bool SUPPORTED = true;
    const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
    PC_HD void operator()(uint32_t lane) const {
      const uint32_t* p = in + (size_t)lane * IN_WORDS;
      const uint32_t* q = p + 4 * FN;
      uint32_t* o = out + (size_t)lane * OUT_WORDS;
      if constexpr (OP == T_DERIVE) { Aff::load_xy(q).store(o + 4 * FN); }
      else if constexpr (OP == T_NEG) { Aff::load(q).neg_if(true).store(o + 4 * FN); }
      else {
        Pt r = Pt::load(p);
        if constexpr (OP == T_MADD) r.add_affine(Aff::load(q));
        else if constexpr (OP == T_ADD) r.add(Pt::load(q));
        else if constexpr (OP == T_DBL) r = r.dbl();
        else if constexpr (OP == T_FROM_AFFINE) r = Pt::from_affine(Aff::load(q));
        r.store(o); r.to_affine().store(o + 4 * FN);
      }
    }
  };
};

// The running sum of a bucket, the twisted Edwards counterpart of Chain30Body.  One lane per index list: in = count | idx[param]
// (idx = table entry in bits 0..5 | sign << 31); aux = 64 resident records (an all-zero one counts as the identity).  The sum starts
// empty; every step is acc.add_affine(tbl[e].neg_if(sign)).
// out = FNV hash of every step's stored words | the final raw X | Y | Z | T | the final to_affine()
template <class G>
struct TeChainBody {
  typedef XyzzD<G> Pt; typedef AffD<G> Aff;
  static constexpr int OUT_WORDS = 1 + Pt::WORDS + Aff::WORDS;
  const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
  PC_HD void operator()(uint32_t lane) const {
    const uint32_t* p = in + (size_t)lane * (1 + param);
    const uint32_t n = p[0] < param ? p[0] : param;
    Pt acc = Pt::infinity();
    uint32_t hash = 0x811c9dc5u;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t e = p[1 + i];
      acc.add_affine(Aff::load(aux + (size_t)(e & 63u) * Aff::WORDS).neg_if((e >> 31) != 0));
      uint32_t w[Pt::WORDS]; acc.store(w);
      for (int k = 0; k < Pt::WORDS; k++) hash = (hash ^ w[k]) * 0x01000193u;
    }
    uint32_t* o = out + (size_t)lane * OUT_WORDS;
    o[0] = hash;
    acc.store(o + 1); acc.to_affine().store(o + 1 + Pt::WORDS);
  }
};

}  // namespace probe
