// Quadratic extension Fq2 = Fq[u] / (u^2 + 1) of a base field whose -1 is a non-residue (BLS12-381, BN254): the coordinate
// field of G2 on the twist.  An element is c0 + c1 u, two Montgomery residues Fd<P> laid out c0 || c1 -- arkworks'
// Fp2 { c0, c1 } in memory -- so 2 N words per element.
//
// It carries the interface AffD / XyzzD (ec.hpp) ask of a coordinate field, so the XYZZ group law is shared with G1.  Every
// value is canonical (both coefficients in [0, p)): none of the lazy [0, 2p) forms of fp32.hpp is used here, and the LAZY_*
// constants below switch the accumulation's lazy paths off for this field.
//
// Product: c0 = a0 b0 + (-a1) b1 and c1 = a0 b1 + a1 b0, each ONE fused multiply pair with one reduction (Fd::mul_add_mul:
// operands canonical, a b + c d < 2 p^2, the bound the canonical fused pair is built for) -- four limb products and two
// reductions, the multiply-add count of Karatsuba's 3 + 3 with fewer additions.
// Square: c0 = (a0 + a1)(a0 - a1), c1 = 2 a0 a1 (canonical sums: Fd::add / sub reduce).
#pragma once
#include "fp32.hpp"

namespace pc {

template <class P>
struct Fq2D {
  typedef Fd<P> F;
  static constexpr int N = 2 * F::N;      // words per element
  static constexpr bool LAZY_OK = false, LAZY_FUSED_OK = false, LAZY_STORE_OK = false;
  F c0, c1;

  static PC_HD Fq2D zero() { Fq2D r; r.c0 = F::zero(); r.c1 = F::zero(); return r; }
  static PC_HD Fq2D one() { Fq2D r; r.c0 = F::one(); r.c1 = F::zero(); return r; }
  static PC_HD Fq2D load(const uint32_t* p) { Fq2D r; r.c0 = F::load(p); r.c1 = F::load(p + F::N); return r; }
  PC_HD void store(uint32_t* p) const { c0.store(p); c1.store(p + F::N); }
  PC_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  PC_HD bool eq(const Fq2D& o) const { return c0.eq(o.c0) && c1.eq(o.c1); }

  PC_HD Fq2D add(const Fq2D& o) const { Fq2D r; r.c0 = c0.add(o.c0); r.c1 = c1.add(o.c1); return r; }
  PC_HD Fq2D sub(const Fq2D& o) const { Fq2D r; r.c0 = c0.sub(o.c0); r.c1 = c1.sub(o.c1); return r; }
  PC_HD Fq2D dbl() const { Fq2D r; r.c0 = c0.dbl(); r.c1 = c1.dbl(); return r; }
  PC_HD Fq2D neg() const { Fq2D r; r.c0 = c0.neg(); r.c1 = c1.neg(); return r; }
  PC_HD Fq2D mul(const Fq2D& o) const {
    Fq2D r;
    r.c0 = c0.mul_add_mul(o.c0, c1.neg(), o.c1);      // a0 b0 - a1 b1: both products below p^2, one reduction
#if defined(__HIP_DEVICE_COMPILE__)
    // the two fused pairs one after the other: interleaved by the scheduler they hold two sets of multiplier temporaries, which took
    // the G2 accumulation (96-word sum + 48-word operand per lane) two registers past the 512 of a lane (.vgpr_spill_count 2 -> 0)
    __builtin_amdgcn_sched_barrier(0);
#endif
    r.c1 = c0.mul_add_mul(o.c1, c1, o.c0);            // a0 b1 + a1 b0
    return r;
  }
  PC_HD Fq2D sqr() const {
    Fq2D r;
    r.c0 = c0.add(c1).mul(c0.sub(c1));                // canonical sum and difference
    r.c1 = c0.dbl().mul(c1);
    return r;
  }
  // a b + c d over Fq2 (the Y coordinate of the XYZZ additions)
  PC_HD Fq2D mul_add_mul(const Fq2D& b, const Fq2D& c, const Fq2D& d) const { return mul(b).add(c.mul(d)); }
  // (a0 - a1 u) / (a0^2 + a1^2); 0 -> 0.  The norm is non-zero for a != 0 because -1 is a non-residue.
  PC_HD Fq2D inv() const {
    const F ni = c0.sqr().add(c1.sqr()).inv();
    Fq2D r; r.c0 = c0.mul(ni); r.c1 = c1.neg().mul(ni);
    return r;
  }
};

}  // namespace pc
