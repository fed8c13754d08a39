// Validation of resident keys on the device: what arkworks does when it reads a key with Validate::Yes.
//
// UniversalParams::deserialize_with_mode(.., Validate::Yes) ends in result.check() (poly-commit/src/kzg10/data_structures.rs:41-49,
// :106-108), and powers_of_g.check() is, per point, is_on_curve() && is_in_correct_subgroup_assuming_on_curve(); an IPA or Hyrax key
// (Vec<G>) read with validation does the same.  One lane per point, flags[i] = 1 for a point that passes:
//
//   SwOnCurveBody<C>         the all-zero encoding of infinity, or both coordinates below the modulus and y^2 = x^3 + b (Montgomery
//                            residues, as resident keys hold them; limbs >= p count as off the curve)
//   SwSubgroupLadderBody<C>  THE DEFINITION: r * P is the point at infinity, r the scalar field's modulus, by the NAF ladder of
//                            TeSubgroupBody (te.hpp) with host-made masks.  All four curves; on BN254 and Pallas (cofactor 1) the ABI
//                            answers without a launch (ark-ec's cofactor_is_one() shortcut), the ladder stays reachable for the tests.
//   Bls12SubgroupBody<C>     the fast path of BLS12-381 and BLS12-377: phi(P) = -[x^2] P with phi(x, y) = (beta' x, y), the test of
//                            eprint 2021/1130 section 6 that ark-bls12-381 and ark-bls12-377 override
//                            is_in_correct_subgroup_assuming_on_curve with.  [x^2] P is two ladders by the 64-bit |x| (63 doublings and 5
//                            or 6 additions each; the second adds an XYZZ point), compared in XYZZ without an inversion.  beta' is the
//                            cube root of unity whose eigenvalue on G1 is -x^2 mod r (validate_constants.h: found on the generator by
//                            tools/gen_constants.py, not assumed).
//   G2OnCurveBody / G2SubgroupBody   the same two checks for BLS12-381 G2 on its twist y^2 = x^3 + 4 (1 + u): the plain ladder by r
//                            (no psi shortcut: G2 keys are short).
//
// The subgroup bodies assume an on-curve point, as arkworks' name says.  `gate` (or null) is the on-curve pass's flags: a lane whose
// gate is 0 stores 0 and runs no ladder, so with both checks a point off the curve fails once.  ValidateTallyBody counts the failures
// and takes the lowest failing index on the device (ordinary vector atomics).
#pragma once
#include "ec.hpp"
#include "validate_constants.h"

namespace pc {

PC_HD void validate_atomic_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, v);
#else
  *p += v;
#endif
}
PC_HD void validate_atomic_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}

// raw limbs below the modulus
template <class P>
PC_HD bool fd_below_modulus(const Fd<P>& a) {
  uint32_t br = 0;                                           // a - p borrows exactly when a < p
  PC_UNROLL for (int k = 0; k < P::N; k++) (void)Fd<P>::sbb(a.l[k], P::MOD[k], br);
  return br != 0;
}

template <class C>
struct SwOnCurveBody {
  typedef AffD<C> Aff;
  typedef typename Aff::Fq Fq;
  const uint32_t* key; uint32_t* flags;
  PC_HD void operator()(uint32_t i) const {
    const Aff p = Aff::load(key + (size_t)i * Aff::WORDS);
    if (p.is_inf()) { flags[i] = 1u; return; }
    bool ok = fd_below_modulus(p.x) && fd_below_modulus(p.y);
    if (ok) ok = p.y.sqr().eq(p.x.sqr().mul(p.x).add(Fq::load(C::B_MONT)));
    flags[i] = ok ? 1u : 0u;
  }
};

// acc = k * p for the NAF of k, most significant digit first (the ladder of TeSubgroupBody over the XYZZ law of ec.hpp)
template <class G, int NW>
PC_HD XyzzD<G> naf_ladder_xyzz(const NafMasks<NW>& naf, const AffD<G>& p) {
  const AffD<G> np = p.neg_if(true);
  XyzzD<G> acc = XyzzD<G>::infinity();
  for (int bit = 32 * (NW + 1) - 1; bit >= 0; bit--) {
    const uint32_t w = bit >> 5, m = 1u << (bit & 31);
    if (!acc.is_inf()) acc = acc.dbl(); else if (!((naf.pos[w] | naf.neg[w]) & m)) continue;
    if (naf.pos[w] & m) acc.add_affine(p); else if (naf.neg[w] & m) acc.add_affine(np);
  }
  return acc;
}

// G: a curve of pc_curve, or G2Of<C> (G2SubgroupBody below)
template <class G>
struct SwSubgroupLadderBody {
  typedef AffD<G> Aff;
  static constexpr int NW = G::FrP::N;
  const uint32_t* key; uint32_t* flags; const uint32_t* gate;
  NafMasks<NW> naf;        // of r
  void set_order() { naf.from_scalar(G::FrP::MOD); }
  PC_HD void operator()(uint32_t i) const {
    if (gate && !gate[i]) { flags[i] = 0u; return; }
    const Aff p = Aff::load(key + (size_t)i * Aff::WORDS);
    flags[i] = (p.is_inf() || naf_ladder_xyzz<G, NW>(naf, p).is_inf()) ? 1u : 0u;
  }
};

template <class C>
struct Bls12SubgroupBody {
  typedef pc_subgroup_constants<C> K;
  typedef XyzzD<C> Pt;
  typedef AffD<C> Aff;
  typedef typename Pt::Fq Fq;
  static_assert(K::HAS_FAST && (K::X_ABS >> 63) == 1, "a BLS12 curve with a 64-bit |x|");
  const uint32_t* key; uint32_t* flags; const uint32_t* gate;
  PC_HD void operator()(uint32_t i) const {
    if (gate && !gate[i]) { flags[i] = 0u; return; }
    const Aff p = Aff::load(key + (size_t)i * Aff::WORDS);
    if (p.is_inf()) { flags[i] = 1u; return; }
    Pt q = Pt::from_affine(p);                               // |x| P, from the bit below the top one
    for (int b = 62; b >= 0; b--) {
      q = q.dbl();
      if ((K::X_ABS >> b) & 1) q.add_affine(p);
    }
    Pt acc = q;                                              // |x| (|x| P) = x^2 P
    for (int b = 62; b >= 0; b--) {
      acc = acc.dbl();
      if ((K::X_ABS >> b) & 1) acc.add(q);
    }
    // phi(P) = (beta' x, y) against -acc = (X / ZZ, -Y / ZZZ); phi(P) is never infinity, so acc = infinity fails
    const bool ok = !acc.is_inf() && p.x.mul(Fq::load(K::BETA_MONT)).mul(acc.ZZ).eq(acc.X) && p.y.mul(acc.ZZZ).eq(acc.Y.neg());
    flags[i] = ok ? 1u : 0u;
  }
};

// BLS12-381 G2: x.c0 || x.c1 || y.c0 || y.c1 on the twist y^2 = x^3 + 4 (1 + u); every coefficient must be below the modulus
template <class C>
struct G2OnCurveBody {
  typedef G2Of<C> G;
  typedef AffD<G> Aff;
  typedef typename Aff::Fq Fq2;
  static_assert(C::B_SMALL == 4, "the twist constant below is b (1 + u)");
  const uint32_t* key; uint32_t* flags;
  PC_HD void operator()(uint32_t i) const {
    const Aff p = Aff::load(key + (size_t)i * Aff::WORDS);
    if (p.is_inf()) { flags[i] = 1u; return; }
    bool ok = fd_below_modulus(p.x.c0) && fd_below_modulus(p.x.c1) && fd_below_modulus(p.y.c0) && fd_below_modulus(p.y.c1);
    if (ok) {
      Fq2 b; b.c0 = Fq2::F::load(C::B_MONT); b.c1 = b.c0;
      ok = p.y.sqr().eq(p.x.sqr().mul(p.x).add(b));
    }
    flags[i] = ok ? 1u : 0u;
  }
};
template <class C> using G2SubgroupBody = SwSubgroupLadderBody<G2Of<C>>;

// flags -> the count of failures, the lowest failing index and (ok != null) one byte per point; *bad = 0 and *first = 0xffffffff before
struct ValidateTallyBody {
  const uint32_t* flags; uint8_t* ok; uint32_t* bad; uint32_t* first;
  PC_HD void operator()(uint32_t i) const {
    const bool pass = flags[i] != 0;
    if (ok) ok[i] = pass ? 1 : 0;
    if (!pass) { validate_atomic_add(bad, 1u); validate_atomic_min(first, i); }
  }
};

}  // namespace pc
