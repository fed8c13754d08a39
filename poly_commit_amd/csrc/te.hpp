// Twisted Edwards group arithmetic, a = -1:  -x^2 + y^2 = 1 + d x^2 y^2  (ed_on_bls12_381 / JubJub, te_constants.h) -- the curve the
// reference runs InnerProductArgPC on (poly-commit/src/ipa_pc/mod.rs:1056-1064, benches/ipa_times.rs:5,16).
//
// a is a square and d is not, so the extended-coordinate formulas of Hisil, Wong, Carter and Dawson are COMPLETE: P + P, P + (-P),
// the identity (0, 1) and the points of order 2, 4 and 8 go through the same instructions as any other pair.  There is no point at
// infinity.  What the MSM templates (msm.hpp) call `infinity()` is the all-zero word pattern of a zero-filled bucket: it means
// "empty", is recognised by Z == 0 (a real point never has Z = 0 under a complete law) and both additions treat it as the
// identity.  The true identity (0, 1, 1, 0) is an ordinary value: a bucket that passes through it (P then -P) simply carries on.
//
//   bucket     extended (X, Y, Z, T), x = X/Z, y = Y/Z, T = XY/Z: 4 N words, the size of an XYZZ bucket
//   base       (x, y, td) with the derived coordinate td = 2 d x y: 3 N words, made once per key (TeDeriveBody).  The mixed addition
//              is then madd-2008-hwcd-3 in 7 multiplications; from the bare (x, y) it would be 9.  An all-zero base (not a curve
//              point) counts as the identity.  The caller's form is always x || y: upload, read-back and every result.
//   formulas   madd-2008-hwcd-3, add-2008-hwcd-3, dbl-2008-hwcd (Explicit-Formulas Database, "Extended coordinates with a = -1")
// The coordinate field is BLS12-381's Fr, 255 bits in 8 words: Fd's LAZY_OK is false for it (4p > 2^256), every value is canonical.
#pragma once
#include "ec.hpp"
#include "host_tail.hpp"
#include "te_constants.h"

namespace pc {

template <class T>
struct AffD<TeOf<T>> {
  typedef Fd<typename T::FqP> Fq;
  static constexpr int XY_WORDS = 2 * Fq::N;
#if PC_TE_DERIVED_TD
  static constexpr int WORDS = 3 * Fq::N;
  Fq x, y, td;
  static PC_HD AffD infinity() { AffD a; a.x = Fq::zero(); a.y = Fq::zero(); a.td = Fq::zero(); return a; }      // the all-zero entry
  static PC_HD AffD identity() { AffD a; a.x = Fq::zero(); a.y = Fq::one(); a.td = Fq::zero(); return a; }
  static PC_HD AffD load(const uint32_t* p) { AffD a; a.x = Fq::load(p); a.y = Fq::load(p + Fq::N); a.td = Fq::load(p + 2 * Fq::N); return a; }
  PC_HD void store(uint32_t* p) const { x.store(p); y.store(p + Fq::N); td.store(p + 2 * Fq::N); }
  // from the caller's x || y (an all-zero pair stays all zero: td = 0)
  static PC_HD AffD from_xy(const Fq& x, const Fq& y) { AffD a; a.x = x; a.y = y; a.td = x.mul(y).mul(Fq::load(T::D2)); return a; }
  PC_HD Fq td_of() const { return td; }
  // -(x, y) = (-x, y): td changes sign with x
  PC_HD AffD neg_if(bool s) const { AffD a; a.x = s ? x.neg() : x; a.y = y; a.td = s ? td.neg() : td; return a; }
#else
  static constexpr int WORDS = 2 * Fq::N;
  Fq x, y;
  static PC_HD AffD infinity() { AffD a; a.x = Fq::zero(); a.y = Fq::zero(); return a; }
  static PC_HD AffD identity() { AffD a; a.x = Fq::zero(); a.y = Fq::one(); return a; }
  static PC_HD AffD load(const uint32_t* p) { AffD a; a.x = Fq::load(p); a.y = Fq::load(p + Fq::N); return a; }
  PC_HD void store(uint32_t* p) const { x.store(p); y.store(p + Fq::N); }
  static PC_HD AffD from_xy(const Fq& x, const Fq& y) { AffD a; a.x = x; a.y = y; return a; }
  PC_HD Fq td_of() const { return x.mul(y).mul(Fq::load(T::D2)); }
  PC_HD AffD neg_if(bool s) const { AffD a; a.x = s ? x.neg() : x; a.y = y; return a; }
#endif
  PC_HD bool is_inf() const { return x.is_zero() && y.is_zero(); }
  static PC_HD AffD load_xy(const uint32_t* p) { return from_xy(Fq::load(p), Fq::load(p + Fq::N)); }
  PC_HD void store_xy(uint32_t* p) const { x.store(p); y.store(p + Fq::N); }
};

template <class T>
struct XyzzD<TeOf<T>> {
  typedef TeOf<T> G;
  typedef Fd<typename T::FqP> Fq;
  static constexpr int WORDS = 4 * Fq::N;
  Fq X, Y, Z, Tc;      // Tc = X Y / Z

  static PC_HD XyzzD infinity() { XyzzD r; r.X = Fq::zero(); r.Y = Fq::zero(); r.Z = Fq::zero(); r.Tc = Fq::zero(); return r; }      // "empty"
  static PC_HD XyzzD identity() { XyzzD r; r.X = Fq::zero(); r.Y = Fq::one(); r.Z = Fq::one(); r.Tc = Fq::zero(); return r; }
  PC_HD bool is_inf() const { return Z.is_zero(); }
  static PC_HD XyzzD from_affine(const AffD<G>& a) {
    if (a.is_inf()) return infinity();
    XyzzD r; r.X = a.x; r.Y = a.y; r.Z = Fq::one(); r.Tc = a.x.mul(a.y); return r;
  }
  static PC_HD XyzzD load(const uint32_t* p) {
    XyzzD r; r.X = Fq::load(p); r.Y = Fq::load(p + Fq::N); r.Z = Fq::load(p + 2 * Fq::N); r.Tc = Fq::load(p + 3 * Fq::N); return r;
  }
  PC_HD void store(uint32_t* p) const { X.store(p); Y.store(p + Fq::N); Z.store(p + 2 * Fq::N); Tc.store(p + 3 * Fq::N); }

  // this += affine, madd-2008-hwcd-3 with the base's td = 2 d x2 y2: 7M.  An empty sum starts from the identity and runs the same
  // instructions (no divergent branch at the first entry of a bucket); an all-zero base is skipped.
  PC_HD void add_affine(const AffD<G>& a) {
    if (a.is_inf()) return;
    if (is_inf()) *this = identity();
    const Fq A = Y.sub(X).mul(a.y.sub(a.x)), B = Y.add(X).mul(a.y.add(a.x));
    const Fq Cc = Tc.mul(a.td_of()), D = Z.dbl();
    const Fq E = B.sub(A), F = D.sub(Cc), Gg = D.add(Cc), H = B.add(A);
    X = E.mul(F); Y = Gg.mul(H); Tc = E.mul(H); Z = F.mul(Gg);
  }
  // this += o, add-2008-hwcd-3: 9M (one of them by the constant 2 d)
  PC_HD void add(const XyzzD& o) {
    if (o.is_inf()) return;
    if (is_inf()) { *this = o; return; }
    const Fq A = Y.sub(X).mul(o.Y.sub(o.X)), B = Y.add(X).mul(o.Y.add(o.X));
    const Fq Cc = Tc.mul(Fq::load(T::D2)).mul(o.Tc), D = Z.mul(o.Z).dbl();
    const Fq E = B.sub(A), F = D.sub(Cc), Gg = D.add(Cc), H = B.add(A);
    X = E.mul(F); Y = Gg.mul(H); Tc = E.mul(H); Z = F.mul(Gg);
  }
  // 2 * this, dbl-2008-hwcd with a = -1: 4M + 4S
  PC_HD XyzzD dbl() const {
    if (is_inf()) return infinity();
    const Fq A = X.sqr(), B = Y.sqr(), Cc = Z.sqr().dbl();
    const Fq D = A.neg(), E = X.add(Y).sqr().sub(A).sub(B), Gg = D.add(B), F = Gg.sub(Cc), H = D.sub(B);
    XyzzD r; r.X = E.mul(F); r.Y = Gg.mul(H); r.Tc = E.mul(H); r.Z = F.mul(Gg);
    return r;
  }
  // (x, y, td); an empty sum gives the all-zero entry
  PC_HD AffD<G> to_affine() const {
    if (is_inf()) return AffD<G>::infinity();
    const Fq zi = Z.inv();
    return AffD<G>::from_xy(X.mul(zi), Y.mul(zi));
  }
};

// resident form of a key from the caller's points: out[i] = (x, y, 2 d x y) from in[i] = x || y.  One kernel at upload.
template <class G>
struct TeDeriveBody {
  typedef AffD<G> Aff;
  const uint32_t* in_xy; uint32_t* out;
  PC_HD void operator()(uint32_t i) const { Aff::load_xy(in_xy + (size_t)i * Aff::XY_WORDS).store(out + (size_t)i * Aff::WORDS); }
};
// and back: out[i] = x || y of the resident point in[i] (read-back)
template <class G>
struct TeStripBody {
  typedef AffD<G> Aff;
  const uint32_t* in; uint32_t* out_xy;
  PC_HD void operator()(uint32_t i) const { Aff::load(in + (size_t)i * Aff::WORDS).store_xy(out_xy + (size_t)i * Aff::XY_WORDS); }
};

// One key fold of InnerProductArgPC::open, ext[i] = key[i] + u * key[half + i] (ipa_pc/mod.rs:699-707: `k_l += k_r * u`), left in
// extended coordinates for TeBatchAffineBody.  u is the round's challenge, shared by every lane: its non-adjacent form is made once on
// the host (NafMasks, ec.hpp) and the lane walks it from the top, a doubling per position and an addition of +-key[half + i] at the
// non-zero digits (a third of them).  The multiplication is exact integer arithmetic on whatever point it is given, as ark-ec's
// `mul_bigint` is: nothing here uses r P = O, so operands outside the prime-order subgroup are multiplied correctly.  An all-zero
// operand counts as the identity; a lane whose two operands both are all zero yields the identity.
template <class G>
struct TeEcFoldBody {
  typedef XyzzD<G> Pt;
  typedef AffD<G> Aff;
  static constexpr int NW = G::FrP::N;
  const uint32_t* key; uint32_t half;
  uint32_t* ext;           // half x Pt::WORDS
  NafMasks<NW> naf;        // of the canonical u
  PC_HD void operator()(uint32_t i) const {
    const Aff kl = Aff::load(key + (size_t)i * Aff::WORDS), kr = Aff::load(key + (size_t)(half + i) * Aff::WORDS);
    const Aff km = kr.neg_if(true);
    Pt acc = Pt::infinity();
    for (int bit = 32 * (NW + 1) - 1; bit >= 0; bit--) {
      const uint32_t w = bit >> 5, m = 1u << (bit & 31);
      if (!acc.is_inf()) acc = acc.dbl(); else if (!((naf.pos[w] | naf.neg[w]) & m)) continue;
      if (naf.pos[w] & m) acc.add_affine(kr); else if (naf.neg[w] & m) acc.add_affine(km);
    }
    acc.add_affine(kl);
    if (acc.is_inf()) acc = Pt::identity();
    acc.store(ext + (size_t)i * Pt::WORDS);
  }
};

// n extended points -> n resident affine points (x, y, td) with ONE inversion per lane of K points (Montgomery's trick along the
// lane's run, what CurveGroup::normalize_batch does in the reference, ipa_pc/mod.rs:706-708): x = X/Z, y = Y/Z, and the derived
// coordinate rebuilt.  Z is never 0 under a complete law; an empty (all-zero) input gives the identity all the same.
template <class G>
struct TeBatchAffineBody {
  typedef XyzzD<G> Pt;
  typedef AffD<G> Aff;
  typedef typename Pt::Fq Fq;
  static constexpr int FN = Fq::N;
  const uint32_t* ext;      // n x Pt::WORDS
  uint32_t* scratch;        // n x Fq (prefix products)
  uint32_t* out;            // n x Aff::WORDS
  uint32_t n, K;
  PC_HD void operator()(uint32_t t) const {
    const uint32_t s = t * K, e = (n - s > K) ? s + K : n;
    Fq run = Fq::one();
    for (uint32_t j = s; j < e; j++) {
      run.store(scratch + (size_t)j * FN);
      const Fq z = Fq::load(ext + (size_t)j * Pt::WORDS + 2 * FN);
      if (!z.is_zero()) run = run.mul(z);
    }
    Fq inv = run.inv();
    for (uint32_t j = e; j-- > s;) {
      const uint32_t* p = ext + (size_t)j * Pt::WORDS;
      const Fq z = Fq::load(p + 2 * FN);
      Aff a = Aff::identity();
      if (!z.is_zero()) {
        const Fq zi = inv.mul(Fq::load(scratch + (size_t)j * FN));
        inv = inv.mul(z);
        a = Aff::from_xy(Fq::load(p).mul(zi), Fq::load(p + FN).mul(zi));
      }
      a.store(out + (size_t)j * Aff::WORDS);
    }
  }
};

// ---- the fold table of a committer key (pc_hip_te_srs_precompute_fold) ------------------------------------------------------
// T[b][j] = 2^b * key[n/2 + j] for b < TE_FOLD_ROWS, row-major in j, every record in the resident form: the first fold of every
// opening multiplies the same upper half of the key by that opening's challenge, and with the doublings stored a fold is one mixed
// addition per non-zero NAF digit (a third of the positions) instead of a doubling per position on top of them.  The curve has no
// endomorphism: there is no GLV split to halve the rows.  253 = the NAF positions of a 252-bit scalar, carry included.
static constexpr uint32_t TE_FOLD_ROWS = 253;

// one row from the one below: ext[j] = 2 * in[j], left in extended coordinates for TeBatchAffineBody (an all-zero record stays empty
// and is normalised to the identity, which the fold adds as it would skip the empty one)
template <class G>
struct TeDblRowBody {
  typedef XyzzD<G> Pt;
  typedef AffD<G> Aff;
  const uint32_t* in; uint32_t* ext;
  PC_HD void operator()(uint32_t j) const {
    const Aff a = Aff::load(in + (size_t)j * Aff::WORDS);
    uint32_t* o = ext + (size_t)j * Pt::WORDS;
    if (a.is_inf()) { for (int w = 0; w < Pt::WORDS; w++) o[w] = 0; return; }
    Pt p; p.X = a.x; p.Y = a.y; p.Z = Pt::Fq::one(); p.Tc = a.x.mul(a.y);
    p.dbl().store(o);
  }
};

// ---- the window table of a key range (pc_hip_te_msm_many) --------------------------------------------------------------------
// T[w][j] = 2^(c w) * key[base_offset + j] for w < Wd, row-major in j, every record in the resident form: with it the many-MSM pass
// puts all windows of a sub-MSM into ONE bucket set (MsmPlan, subs > 0; HyraxPC::commit, hyrax/mod.rs:233-242).  Row w + 1 is row w
// doubled c times in extended coordinates, then one TeBatchAffineBody over the row -- TeDblRowBody with every c-th row kept.  The
// doubling is dbl-2008-hwcd under the complete law: points of order 2, 4 and 8 and the identity go through the same instructions; an
// all-zero record stays empty and is normalised to the identity, which the accumulation adds as it would skip the empty one.
template <class G>
struct TeWindowRowBody {
  typedef XyzzD<G> Pt;
  typedef AffD<G> Aff;
  const uint32_t* in; uint32_t* ext; uint32_t c;
  PC_HD void operator()(uint32_t j) const {
    const Aff a = Aff::load(in + (size_t)j * Aff::WORDS);
    uint32_t* o = ext + (size_t)j * Pt::WORDS;
    if (a.is_inf()) { for (int w = 0; w < Pt::WORDS; w++) o[w] = 0; return; }
    Pt p; p.X = a.x; p.Y = a.y; p.Z = Pt::Fq::one(); p.Tc = a.x.mul(a.y);
    for (uint32_t k = 0; k < c; k++) p = p.dbl();
    p.store(o);
  }
};

// The whole table on the backend's queue: row 0 is the range as it is (an all-zero record stays all zero there: the accumulation skips
// it), row w + 1 is row w through TeWindowRowBody and TeBatchAffineBody with K points per inversion.  ext: m extended points,
// scratch: m Fq, both the caller's.  Returns with everything queued.
template <class G, class Backend>
void te_window_table(Backend& be, const uint32_t* b0, size_t m, uint32_t c, uint32_t Wd, uint32_t* table, uint32_t* ext, uint32_t* scratch, uint32_t K) {
  const size_t row_words = m * (size_t)AffD<G>::WORDS;
  be.copy_d2d(table, b0, row_words * 4);
  for (uint32_t w = 0; w + 1 < Wd; w++) {
    TeWindowRowBody<G> d{table + w * row_words, ext, c};
    be.launch(d, m);
    TeBatchAffineBody<G> nb{ext, scratch, table + (w + 1) * row_words, (uint32_t)m, K};
    be.launch(nb, (m + K - 1) / K);
  }
}

// the non-zero NAF digits of a fold challenge, one entry each: the table row in bits 0..14, bit 15 set for digit -1.  Made once on
// the host and passed by value: every lane of a wave walks the same list (no divergence, the entries come through the scalar unit).
struct TeFoldDigits {
  static constexpr uint32_t MAX = 128;       // a NAF of 253 positions has at most 127 non-zero digits
  uint32_t count;
  uint16_t d[MAX];
  // false: a digit at or above `rows` (the caller runs the ladder)
  template <int NW>
  bool from_naf(const NafMasks<NW>& naf, uint32_t rows) {
    count = 0;
    for (uint32_t bit = 0; bit < 32u * (NW + 1); bit++) {
      const uint32_t w = bit >> 5, m = 1u << (bit & 31);
      if (!((naf.pos[w] | naf.neg[w]) & m)) continue;
      if (bit >= rows || count >= MAX) return false;
      d[count++] = (uint16_t)(bit | ((naf.neg[w] & m) ? 0x8000u : 0u));
    }
    return true;
  }
};

// ext[i] = key[i] + sum over the digits of +-T[row][i]: the same integer combination as TeEcFoldBody's ladder (exact for operands of any
// order; nothing uses r P = O), so the normalised result is the same, bit for bit.  The next row's record is loaded while the current
// addition runs (as the accumulate's StageRegs does for its next base): consecutive lanes read consecutive 96-byte records of one
// row.  u = 0: no digits, key[i] itself; an all-zero record counts as the identity.
template <class G>
struct TeTableFoldBody {
  typedef XyzzD<G> Pt;
  typedef AffD<G> Aff;
  const uint32_t* key; const uint32_t* tbl; uint32_t half;
  uint32_t* ext;           // half x Pt::WORDS
  TeFoldDigits dg;
  PC_HD void operator()(uint32_t i) const {
    Pt acc = Pt::from_affine(Aff::load(key + (size_t)i * Aff::WORDS));
    const uint32_t* col = tbl + (size_t)i * Aff::WORDS;
    const size_t row = (size_t)half * Aff::WORDS;
    Aff nxt = dg.count ? Aff::load(col + (size_t)(dg.d[0] & 0x7fffu) * row) : Aff::infinity();
    for (uint32_t k = 0; k < dg.count; k++) {
      const Aff cur = nxt.neg_if((dg.d[k] >> 15) != 0);
      if (k + 1 < dg.count) nxt = Aff::load(col + (size_t)(dg.d[k + 1] & 0x7fffu) * row);
      acc.add_affine(cur);
    }
    if (acc.is_inf()) acc = Pt::identity();
    acc.store(ext + (size_t)i * Pt::WORDS);
  }
};

// flags[i] = 1 if r * key[i] is the identity (key[i] lies in the prime-order subgroup), else 0: the NAF ladder of the group order r,
// its masks made on the host.  The fixed-key rounds of an opening reduce products of challenges modulo r before they meet a base,
// which is exact only for such points; the ABI itself takes any curve point.  An all-zero entry counts as the identity.
template <class G>
struct TeSubgroupBody {
  typedef XyzzD<G> Pt;
  typedef AffD<G> Aff;
  static constexpr int NW = G::FrP::N;
  const uint32_t* key; uint32_t* flags;
  NafMasks<NW> naf;        // of r
  PC_HD void operator()(uint32_t i) const {
    const Aff p = Aff::load(key + (size_t)i * Aff::WORDS), np = p.neg_if(true);
    Pt acc = Pt::infinity();
    for (int bit = 32 * (NW + 1) - 1; bit >= 0; bit--) {
      const uint32_t w = bit >> 5, m = 1u << (bit & 31);
      if (!acc.is_inf()) acc = acc.dbl(); else if (!((naf.pos[w] | naf.neg[w]) & m)) continue;
      if (naf.pos[w] & m) acc.add_affine(p); else if (naf.neg[w] & m) acc.add_affine(np);
    }
    // the identity is X = 0 and Y = Z ((0, -1) of order 2 has X = 0 too)
    flags[i] = (acc.is_inf() || (acc.X.is_zero() && acc.Y.sub(acc.Z).is_zero())) ? 1u : 0u;
  }
};

// ---- the host side (64-bit limbs): the MSM's Horner tail and the handful-of-points utilities --------------------------------
namespace host64 {
template <class T>
struct Xyzz64<TeOf<T>> {
  typedef F64<typename T::FqP> Fq;
  static constexpr int FW = Fq::WORDS;
  Fq X, Y, Z, Tc;
  static Xyzz64 infinity() { Xyzz64 r; r.X = r.Y = r.Z = r.Tc = Fq::zero(); return r; }      // "empty", as on the device
  bool is_inf() const { return Z.is_zero(); }
  void store(uint32_t* p) const { X.store(p); Y.store(p + FW); Z.store(p + 2 * FW); Tc.store(p + 3 * FW); }
  static Xyzz64 load(const uint32_t* p) { Xyzz64 r; r.X = Fq::load(p); r.Y = Fq::load(p + FW); r.Z = Fq::load(p + 2 * FW); r.Tc = Fq::load(p + 3 * FW); return r; }
  // the caller's x || y (2 * FW words; all zero: counts as the identity)
  static Xyzz64 from_affine(const uint32_t* xy) {
    bool zero = true; for (int i = 0; i < 2 * FW; i++) zero &= xy[i] == 0;
    if (zero) return infinity();
    Xyzz64 r; r.X = Fq::load(xy); r.Y = Fq::load(xy + FW); r.Z = Fq::one(); r.Tc = r.X.mul(r.Y);
    return r;
  }
  Xyzz64 dbl() const {   // dbl-2008-hwcd, a = -1
    if (is_inf()) return infinity();
    const Fq A = X.sqr(), B = Y.sqr(), Cc = Z.sqr().dbl();
    const Fq D = Fq::zero().sub(A), E = X.add(Y).sqr().sub(A).sub(B), G = D.add(B), F = G.sub(Cc), H = D.sub(B);
    Xyzz64 r; r.X = E.mul(F); r.Y = G.mul(H); r.Tc = E.mul(H); r.Z = F.mul(G);
    return r;
  }
  void add(const Xyzz64& o) {   // add-2008-hwcd-3
    if (o.is_inf()) return;
    if (is_inf()) { *this = o; return; }
    const Fq A = Y.sub(X).mul(o.Y.sub(o.X)), B = Y.add(X).mul(o.Y.add(o.X));
    const Fq Cc = Tc.mul(Fq::load(T::D2)).mul(o.Tc), D = Z.mul(o.Z).dbl();
    const Fq E = B.sub(A), F = D.sub(Cc), G = D.add(Cc), H = B.add(A);
    X = E.mul(F); Y = G.mul(H); Tc = E.mul(H); Z = F.mul(G);
  }
  // affine x || y (Montgomery); an empty sum is the identity (0, 1)
  void store_affine(uint32_t* out) const {
    if (is_inf()) { Fq::zero().store(out); Fq::one().store(out + FW); return; }
    const Fq zi = Z.inv();
    X.mul(zi).store(out); Y.mul(zi).store(out + FW);
  }
  // the sum of `count` points given as x || y
  static void points_sum(const uint32_t* pts, size_t count, uint32_t* out_affine) {
    Xyzz64 acc = infinity();
    for (size_t i = 0; i < count; i++) acc.add(from_affine(pts + i * 2 * FW));
    acc.store_affine(out_affine);
  }
  // count extended points -> count affine points x || y with one inversion
  static void batch_to_affine(const uint32_t* ext, size_t count, uint32_t* out_affine) {
    std::vector<Fq> prefix(count);
    Fq run = Fq::one();
    for (size_t i = 0; i < count; i++) {
      prefix[i] = run;
      const Xyzz64 p = load(ext + i * 4 * FW);
      if (!p.is_inf()) run = run.mul(p.Z);
    }
    Fq inv = run.inv();
    for (size_t i = count; i-- > 0;) {
      const Xyzz64 p = load(ext + i * 4 * FW);
      uint32_t* o = out_affine + i * 2 * FW;
      if (p.is_inf()) { Fq::zero().store(o); Fq::one().store(o + FW); continue; }
      const Fq zi = inv.mul(prefix[i]);
      inv = inv.mul(p.Z);
      p.X.mul(zi).store(o); p.Y.mul(zi).store(o + FW);
    }
  }
};
// x || y is the identity (0, 1) in Montgomery form, arkworks' Affine::zero()
template <class T>
inline bool te_is_identity(const uint32_t* xy) {
  typedef F64<typename T::FqP> Fq;
  uint32_t one[Fq::WORDS]; Fq::one().store(one);
  uint32_t acc = 0;
  for (int i = 0; i < Fq::WORDS; i++) acc |= xy[i] | (xy[Fq::WORDS + i] ^ one[i]);
  return acc == 0;
}
}  // namespace host64
}  // namespace pc
