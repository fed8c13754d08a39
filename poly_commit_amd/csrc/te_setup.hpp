// InnerProductArgPC::sample_generators on the device (poly-commit/src/ipa_pc/mod.rs:302-325) for ed_on_bls12_381: generator i is
//     8 * from_random_bytes(D(name || le64(i)))                    or, while that is None, for j = 0, 1, 2, ...
//     8 * from_random_bytes(D(name || le64(i) || le64(j)))         (the retry with j = 0 is another message than the first digest)
// with D = Blake2s256 (hash.hpp) and G = twisted_edwards::Affine, then normalize_batch (TeBatchAffineBody, te.hpp).  One lane per index.
//
// from_random_bytes is restated from the published behaviour of ark-ec / ark-ff 0.5 (the versions the reference pins) and, like the
// transcript conventions of host/transcript.hpp and te_ipa.py, NOT confirmed against the crates:
//   the 32 digest bytes are a little-endian integer v.  TEFlags has one flag bit and the modulus 255: 256 bits, the flag is bit 255.
//   y = v mod 2^255; None at y >= q.  x^2 = (1 - y^2) / (a - d y^2) with a = -1: the denominator is never 0 (a / d is a non-square);
//   None where x^2 is a non-square, 0 counts as a square with root 0.  Of the two roots the LARGER canonical integer is taken when
//   the flag is set and the smaller when it is clear, so it does not matter which of them the square root returns.
//
// The square root.  q - 1 = 2^32 t with t odd (te_constants.h: SQRT_S, SQRT_EXP = (t - 1) / 2, SQRT_C = z^t of order 2^32).  For
// n = u / w the division and the first power of Tonelli-Shanks are one exponentiation (the sqrt_ratio of RFC 9380, F.2.1.1):
//     A = w^(2^32 - 1),  E = (u w^(2^33 - 1))^((t - 1) / 2) A = n^((t - 1) / 2) / w        [ (w^(2^33))^((t - 1) / 2) = w^(-2^32) ]
//     r = E u = n^((t + 1) / 2),   tt = r E w = n^t,   r^2 = n tt
// and the loop of Tonelli and Shanks removes tt, whose order is 2^k with k <= 32: n is a square exactly when k <= 31.  The decision is
// exact, nothing is probabilistic.  At most 32 rounds of at most 32 squarings each.
#pragma once
#include "setup_digest.hpp"
#include "te.hpp"

namespace pc {

static constexpr uint32_t TE_SETUP_MAX_DIGESTS = 256;  // the cap of a lane's retry loop (a rejection has probability about 0.55)

// root of u / w (w != 0) into *root and true, or false where u / w is a non-square; u = 0 gives the root 0
template <class T>
PC_HD bool te_sqrt_ratio(const Fd<typename T::FqP>& u, const Fd<typename T::FqP>& w, Fd<typename T::FqP>* root) {
  typedef Fd<typename T::FqP> Fq;
  if (u.is_zero()) { *root = Fq::zero(); return true; }
  Fq A = w;                                                  // w^(2^k - 1), k = 1 .. 32
  for (int k = 1; k < T::SQRT_S; k++) A = A.sqr().mul(w);
  const Fq base = A.sqr().mul(w).mul(u);                     // u w^(2^33 - 1)
  Fq E = Fq::one();
  for (int wd = T::SQRT_EXP_WORDS - 1; wd >= 0; wd--) {
    const uint32_t e = T::SQRT_EXP[wd];
    for (int b = 31; b >= 0; b--) {
      E = E.sqr();
      if ((e >> b) & 1) E = E.mul(base);
    }
  }
  E = E.mul(A);
  Fq r = E.mul(u);
  Fq tt = r.mul(E.mul(w));
  const Fq one = Fq::one();
  Fq c = Fq::load(T::SQRT_C);
  int m = T::SQRT_S;
  // invariants: r^2 = n tt, c has order exactly 2^m, and from the second round on the order of tt is below 2^m
  for (int round = 0; round < T::SQRT_S && !tt.eq(one); round++) {
    int i = 0;
    Fq x = tt;
    while (i < m && !x.eq(one)) { x = x.sqr(); i++; }
    if (i >= m) return false;                                // the order of tt is 2^m: only at m = 32, n is a non-square
    Fq b = c;
    for (int k = 0; k < m - i - 1; k++) b = b.sqr();
    m = i; c = b.sqr(); tt = tt.mul(c); r = r.mul(b);
  }
  *root = r;
  return true;
}

enum : uint32_t { TE_TRY_ACCEPT = 0, TE_TRY_RANGE = 1, TE_TRY_NON_SQUARE = 2 };

// twisted_edwards::Affine::from_random_bytes on a digest (8 words whose little-endian image is the 32 bytes): x and y in Montgomery form
template <class T>
PC_HD uint32_t te_from_random_bytes(const uint32_t* dig, Fd<typename T::FqP>* x, Fd<typename T::FqP>* y) {
  typedef Fd<typename T::FqP> Fq;
  typedef typename T::FqP P;
  static_assert(P::N == 8 && P::BITS == 255, "one flag bit on top of a 255-bit coordinate");
  const bool flag = (dig[7] >> 31) != 0;
  Fq yc;
  PC_UNROLL for (int k = 0; k < 8; k++) yc.l[k] = dig[k];
  yc.l[7] &= 0x7fffffffu;
  uint32_t br = 0;                                           // y - q borrows exactly when y < q
  PC_UNROLL for (int k = 0; k < 8; k++) (void)Fq::sbb(yc.l[k], P::MOD[k], br);
  if (!br) return TE_TRY_RANGE;
  const Fq ym = yc.to_mont(), y2 = ym.sqr(), one = Fq::one();
  const Fq u = one.sub(y2), w = one.add(y2.mul(Fq::load(T::D))).neg();      // a - d y^2 with a = -1
  Fq r;
  if (!te_sqrt_ratio<T>(u, w, &r)) return TE_TRY_NON_SQUARE;
  // r > q - r as canonical integers  <=>  r > (q - 1) / 2
  const Fq rc = r.from_mont();
  uint32_t b2 = 0;                                           // (q - 1) / 2 - r borrows exactly when r is the larger root
  PC_UNROLL for (int k = 0; k < 8; k++) (void)Fq::sbb((P::MOD[k] >> 1) | (k < 7 ? P::MOD[k < 7 ? k + 1 : 7] << 31 : 0u), rc.l[k], b2);
  *x = ((b2 != 0) != flag) ? r.neg() : r;
  *y = ym;
  return TE_TRY_ACCEPT;
}

// generator first + lane, times the cofactor, left in extended coordinates for TeBatchAffineBody; digests[lane] = the digests it
// consumed (1: the first one was accepted).  A lane that finds no point within TE_SETUP_MAX_DIGESTS digests stores the identity and
// raises *failed: the loop is bounded whatever the hash does.
template <class G>
struct TeSampleBody {
  typedef typename G::Curve T;
  typedef XyzzD<G> Pt;
  typedef typename Pt::Fq Fq;
  TeSetupName name;
  uint64_t first;
  uint32_t* ext;           // lanes x Pt::WORDS
  uint32_t* digests;       // lanes
  uint32_t* failed;        // one word, zeroed by the caller
  PC_HD void operator()(uint32_t lane) const {
    const uint64_t i = first + lane;
    Fq x, y;
    uint32_t dig[8], used = 0;
    bool ok = false;
    while (!ok && used < TE_SETUP_MAX_DIGESTS) {
      te_setup_digest(name, i, used != 0, used ? used - 1 : 0, dig);
      used++;
      ok = te_from_random_bytes<T>(dig, &x, &y) == TE_TRY_ACCEPT;
    }
    Pt p = Pt::identity();
    if (ok) {
      p.X = x; p.Y = y; p.Z = Fq::one(); p.Tc = x.mul(y);
      PC_UNROLL for (int k = 1; k < T::COFACTOR; k *= 2) p = p.dbl();      // mul_by_cofactor_to_group: 8 = 2^3
    } else *failed = 1u;
    p.store(ext + (size_t)lane * Pt::WORDS);
    digests[lane] = used;
  }
};

}  // namespace pc
