// sample_generators on the device for the short Weierstrass curves of pc_curve (BLS12-381, BN254, Pallas, BLS12-377; y^2 = x^3 + b):
// InnerProductArgPC's (poly-commit/src/ipa_pc/mod.rs:302-325) and HyraxPC::setup's copy of the same loop (hyrax/mod.rs:119-168).
// Generator i is
//     h * from_random_bytes(D(name || le64(i)))                    or, while that is None, for j = 0, 1, 2, ...
//     h * from_random_bytes(D(name || le64(i) || le64(j)))
// with D = Blake2s256 (setup_digest.hpp), G = short_weierstrass::Affine, h the cofactor (mul_by_cofactor_to_group), then
// normalize_batch (XyzzBatchAffineBody, ipa.hpp).  One lane per index, as te_setup.hpp does it for ed_on_bls12_381.
//
// from_random_bytes is restated from the published behaviour of ark-ec / ark-ff 0.5 (the versions the reference pins) and, like the
// twisted Edwards restatement of te_setup.hpp and the point encodings of serialize.hpp, NOT confirmed against the crates:
//   Fp::from_random_bytes_with_flags::<SWFlags> copies the 32 digest bytes into a buffer of ceil((bits + 2) / 8) bytes and reads the two
//   flag bits from the top of the buffer's LAST byte:
//     BLS12-381 (381 bits), BLS12-377 (377 bits)   48 bytes: byte 47 is zero, the flags are clear; x is the 256-bit digest, always < p
//     Pallas (255 bits)                             33 bytes: byte 32 is zero, the flags are clear; x = digest mod 2^255, None at x >= p
//     BN254 (254 bits)                              32 bytes: the flags are bits 7 and 6 of byte 31; x = digest mod 2^254, None at x >= p
//   flags: 0x80 YIsNegative, 0x40 PointAtInfinity, both: None.  PointAtInfinity gives the identity at x = 0 and None otherwise.
//   Then get_point_from_x_unchecked: y^2 = x^3 + b, None at a non-square (0 is a square with root 0), and of the two roots the one the
//   flag names.  WHICH root a flag names is sw_pick_root below, the one place that decides it: the root SrsDecodeBody (serialize.hpp)
//   takes for the same flag of a compressed point -- YIsPositive (no flag) is the root with y <= -y as canonical integers, YIsNegative
//   the other; ark-ec maps flag to root through the same call in both places.  Either root gives a valid key: only bit parity with the
//   keys arkworks makes rests on this choice.
//
// The square root (setup_constants.h).  p = 3 mod 4 (BLS12-381, BN254): y = n^((p + 1) / 4) and the check y^2 = n.  Pallas (p - 1 =
// 2^32 t) and BLS12-377 (2^46 t): Tonelli and Shanks from w = n^((t - 1) / 2), r = n w, tt = r w = n^t, with the exact decision of
// te_sqrt_ratio: the order of tt is 2^k with k <= SQRT_S, and n is a square exactly when k < SQRT_S.  No inversion: there is no ratio.
//
// The cofactor: 1 for BN254 and Pallas (the point is stored as it is); 126 and 125 bits for the two BLS12 curves, most significant bit
// first by doubling and mixed addition in XYZZ.  The identity in gives the identity out.
#pragma once
#include "ec.hpp"
#include "setup_constants.h"
#include "setup_digest.hpp"

namespace pc {

static constexpr uint32_t SW_SETUP_MAX_DIGESTS = 256;   // the cap of a lane's retry loop (a rejection has probability 0.5 .. 0.81: 0.81^256 = 4e-24)

// a root of n into *root and true, or false where n is a non-square; 0 gives the root 0 (Montgomery in and out)
template <class FqP>
PC_HD bool sw_sqrt(const Fd<FqP>& n, Fd<FqP>* root) {
  typedef Fd<FqP> Fq;
  typedef pc_sqrt_constants<FqP> K;
  static_assert(K::SQRT_S == FqP::TWO_ADICITY, "the two generated headers describe one field");
  if (n.is_zero()) { *root = Fq::zero(); return true; }
  Fq w = n;                                                  // n^SQRT_EXP, from the bit below the exponent's highest
  for (int b = K::SQRT_EXP_BITS - 2; b >= 0; b--) {
    w = w.sqr();
    if ((K::SQRT_EXP[b >> 5] >> (b & 31)) & 1) w = w.mul(n);
  }
  if constexpr (K::SQRT_S == 1) {
    *root = w;
    return w.sqr().eq(n);
  } else {
    Fq r = n.mul(w);
    Fq tt = r.mul(w);
    const Fq one = Fq::one();
    Fq c = Fq::load(K::SQRT_C);
    int m = K::SQRT_S;
    // invariants: r^2 = n tt, c has order exactly 2^m, and from the second round on the order of tt is below 2^m
    for (int round = 0; round < K::SQRT_S && !tt.eq(one); round++) {
      int i = 0;
      Fq x = tt;
      while (i < m && !x.eq(one)) { x = x.sqr(); i++; }
      if (i >= m) return false;                              // the order of tt is 2^m: only at m = SQRT_S, n is a non-square
      Fq b = c;
      for (int k = 0; k < m - i - 1; k++) b = b.sqr();
      m = i; c = b.sqr(); tt = tt.mul(c); r = r.mul(b);
    }
    *root = r;
    return true;
  }
}

// THE mapping from SWFlags to a root (see the header comment: restated, not confirmed against ark-ec).  r: either root of y^2 = n.
// YIsPositive (want_larger false) is the root with y <= -y as canonical integers, YIsNegative (true) the other; y = 0 is both.
template <class FqP>
PC_HD Fd<FqP> sw_pick_root(const Fd<FqP>& r, bool want_larger) {
  const Fd<FqP> nr = r.neg();
  const Fd<FqP> rc = r.from_mont(), nc = nr.from_mont();
  bool r_is_larger = false;                                  // r > -r
  for (int i = FqP::N - 1; i >= 0; i--) { if (rc.l[i] != nc.l[i]) { r_is_larger = rc.l[i] > nc.l[i]; break; } }
  return fq_sel(r_is_larger == want_larger, r, nr);          // limb by limb: a select of whole elements went through scratch memory
}

enum : uint32_t { SW_TRY_ACCEPT = 0, SW_TRY_RANGE = 1, SW_TRY_NON_SQUARE = 2, SW_TRY_FLAGS = 3 };

// short_weierstrass::Affine::from_random_bytes on a digest (8 words whose little-endian image is the 32 bytes): x and y in Montgomery
// form; the identity, which only BN254's flag bits can ask for, is accepted as x = y = 0
template <class C>
PC_HD uint32_t sw_from_random_bytes(const uint32_t* dig, Fd<typename C::FqP>* x, Fd<typename C::FqP>* y) {
  typedef typename C::FqP P;
  typedef Fd<P> Fq;
  static_assert(P::N >= 8 && P::BITS >= 254, "a 32-byte digest fills at most the low 8 words");
  constexpr bool FLAGS_IN_DIGEST = (P::BITS + 2 + 7) / 8 <= 32;      // the buffer's last byte is byte 31 of the digest
  bool y_negative = false, infinity = false;
  if constexpr (FLAGS_IN_DIGEST) { y_negative = (dig[7] >> 31) != 0; infinity = ((dig[7] >> 30) & 1u) != 0; }
  Fq xc = Fq::zero();
  PC_UNROLL for (int k = 0; k < 8; k++) xc.l[k] = dig[k];
  if constexpr (P::BITS < 256) {
    xc.l[7] &= 0xffffffffu >> (256 - P::BITS);               // digest mod 2^BITS
    uint32_t br = 0;                                         // x - p borrows exactly when x < p
    PC_UNROLL for (int k = 0; k < P::N; k++) (void)Fq::sbb(xc.l[k], P::MOD[k], br);
    if (!br) return SW_TRY_RANGE;
  }
  if (y_negative && infinity) return SW_TRY_FLAGS;
  if (infinity) {
    if (!xc.is_zero()) return SW_TRY_FLAGS;
    *x = Fq::zero(); *y = Fq::zero();
    return SW_TRY_ACCEPT;
  }
  const Fq xm = xc.to_mont();
  const Fq rhs = xm.sqr().mul(xm).add(Fq::load(C::B_MONT));
  Fq r;
  if (!sw_sqrt<P>(rhs, &r)) return SW_TRY_NON_SQUARE;
  *x = xm;
  *y = sw_pick_root<P>(r, y_negative);
  return SW_TRY_ACCEPT;
}

// mul_by_cofactor_to_group: h * a in XYZZ, most significant bit of h first; (0, 0) in, infinity out
template <class C>
PC_HD XyzzD<C> sw_mul_by_cofactor(const AffD<C>& a) {
  typedef pc_cofactor_constants<C> K;
  XyzzD<C> acc = XyzzD<C>::from_affine(a);
  for (int b = K::COFACTOR_BITS - 2; b >= 0; b--) {
    acc = acc.dbl();
    if ((K::COFACTOR[b >> 5] >> (b & 31)) & 1) acc.add_affine(a);
  }
  return acc;
}

// the point of index i before the cofactor: the retry loop, capped; returns the digests consumed, *ok false at the cap
template <class C>
PC_HD uint32_t sw_sample_point(const TeSetupName& name, uint64_t i, AffD<C>* a, bool* ok) {
  uint32_t dig[8], used = 0;
  *ok = false;
  while (!*ok && used < SW_SETUP_MAX_DIGESTS) {
    te_setup_digest(name, i, used != 0, used ? used - 1 : 0, dig);
    used++;
    *ok = sw_from_random_bytes<C>(dig, &a->x, &a->y) == SW_TRY_ACCEPT;
  }
  if (!*ok) *a = AffD<C>::infinity();
  return used;
}

// Generator first + lane BEFORE the cofactor, as an affine point (the identity as the all-zero point).  For a curve of cofactor 1 that
// is the generator itself and `out` is the key; for the others SwCofactorBody follows in a launch of its own: with the XYZZ sum of the
// cofactor ladder beside the exponentiation's operands the 12-limb instantiations spilled (DESIGN.md has the figures of both forms).
// digests[lane] = the digests the lane consumed (1: the first one was accepted).  A lane that finds no point within
// SW_SETUP_MAX_DIGESTS digests stores the identity and raises *failed: the loop is bounded whatever the hash does.
template <class C>
struct SwSampleBody {
  static constexpr bool COFACTOR_ONE = pc_cofactor_constants<C>::COFACTOR_BITS == 1;
  TeSetupName name;
  uint64_t first;
  uint32_t* out;           // lanes x AffD<C>::WORDS
  uint32_t* digests;       // lanes
  uint32_t* failed;        // one word, zeroed by the caller
  PC_HD void operator()(uint32_t lane) const {
    AffD<C> a;
    bool ok;
    const uint32_t used = sw_sample_point<C>(name, first + lane, &a, &ok);
    if (!ok) *failed = 1u;
    a.store(out + (size_t)lane * AffD<C>::WORDS);
    digests[lane] = used;
  }
};

// ext[lane] = cofactor * aff[lane] in XYZZ, for XyzzBatchAffineBody
template <class C>
struct SwCofactorBody {
  const uint32_t* aff;     // lanes x AffD<C>::WORDS
  uint32_t* ext;           // lanes x XyzzD<C>::WORDS
  PC_HD void operator()(uint32_t lane) const {
    sw_mul_by_cofactor<C>(AffD<C>::load(aff + (size_t)lane * AffD<C>::WORDS)).store(ext + (size_t)lane * XyzzD<C>::WORDS);
  }
};

}  // namespace pc
