// Host-side finish of an MSM: the Horner fold of the <= W*levels window/level sums and the
// single inversion to affine.  This is a ~255-doubling dependency chain; one CPU core
// (64-bit limbs, unsigned __int128) runs it in ~0.15 ms where one GPU lane would need
// milliseconds.  Input/outputs are the same little-endian Montgomery bytes the device uses.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "field_constants.h"

namespace pc {
namespace host64 {

typedef unsigned __int128 u128;

template <class P>   // P = one of the 32-bit-limb constant structs, N even
struct F64 {
  static constexpr int N = P::N / 2;
  static constexpr int WORDS = P::N;      // 32-bit words per element
  uint64_t l[N];
  static constexpr uint64_t mod(int i) { return (uint64_t)P::MOD[2 * i] | ((uint64_t)P::MOD[2 * i + 1] << 32); }
  static constexpr uint64_t inv64() {   // -p^-1 mod 2^64 by Newton iteration
    uint64_t p0 = mod(0), x = 1;
    for (int i = 0; i < 6; i++) x *= 2 - p0 * x;
    return (uint64_t)0 - x;
  }
  static F64 zero() { F64 r; memset(r.l, 0, sizeof(r.l)); return r; }
  static F64 one() { F64 r; memcpy(r.l, P::ONE, sizeof(r.l)); return r; }
  static F64 load(const uint32_t* p) { F64 r; memcpy(r.l, p, sizeof(r.l)); return r; }
  void store(uint32_t* p) const { memcpy(p, l, sizeof(l)); }
  bool is_zero() const { uint64_t a = 0; for (int i = 0; i < N; i++) a |= l[i]; return a == 0; }
  static bool geq(const uint64_t* a) {
    for (int i = N - 1; i >= 0; i--) { if (a[i] > mod(i)) return true; if (a[i] < mod(i)) return false; }
    return true;
  }
  static void subm(uint64_t* a) {
    u128 br = 0;
    for (int i = 0; i < N; i++) { u128 d = (u128)a[i] - mod(i) - (uint64_t)br; a[i] = (uint64_t)d; br = (d >> 64) & 1; }
  }
  F64 add(const F64& o) const {
    F64 r; u128 c = 0;
    for (int i = 0; i < N; i++) { c += (u128)l[i] + o.l[i]; r.l[i] = (uint64_t)c; c >>= 64; }
    if (geq(r.l)) subm(r.l);
    return r;
  }
  F64 sub(const F64& o) const {
    F64 r; u128 br = 0;
    for (int i = 0; i < N; i++) { u128 d = (u128)l[i] - o.l[i] - (uint64_t)br; r.l[i] = (uint64_t)d; br = (d >> 64) & 1; }
    if (br) { u128 c = 0; for (int i = 0; i < N; i++) { c += (u128)r.l[i] + mod(i); r.l[i] = (uint64_t)c; c >>= 64; } }
    return r;
  }
  F64 dbl() const { return add(*this); }
  F64 mul(const F64& o) const {
    constexpr uint64_t INV = inv64();
    uint64_t t[N + 2];
    for (int i = 0; i < N + 2; i++) t[i] = 0;
    for (int i = 0; i < N; i++) {
      u128 c = 0;
      for (int j = 0; j < N; j++) { c += (u128)l[j] * o.l[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
      c += t[N]; t[N] = (uint64_t)c; t[N + 1] = (uint64_t)(c >> 64);
      uint64_t m = t[0] * INV;
      c = (u128)m * mod(0) + t[0]; c >>= 64;
      for (int j = 1; j < N; j++) { c += (u128)m * mod(j) + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
      c += t[N]; t[N - 1] = (uint64_t)c; t[N] = t[N + 1] + (uint64_t)(c >> 64);
    }
    F64 r; for (int i = 0; i < N; i++) r.l[i] = t[i];
    if (t[N] || geq(r.l)) subm(r.l);
    return r;
  }
  F64 sqr() const { return mul(*this); }
  F64 inv() const {   // a^(p-2)
    uint64_t e[N]; u128 br = 2;
    for (int i = 0; i < N; i++) { u128 d = (u128)mod(i) - (uint64_t)br; e[i] = (uint64_t)d; br = (d >> 64) & 1; }
    F64 r = one();
    for (int i = N * 64 - 1; i >= 0; i--) { r = r.sqr(); if ((e[i / 64] >> (i % 64)) & 1) r = r.mul(*this); }
    return r;
  }
};

// Fq2 = Fq[u] / (u^2 + 1) on the host (the device's Fq2D, fp2.hpp: same layout c0 || c1, same canonical values): the coordinates
// of the G2 partial sums.  The inversion is (a0 - a1 u) / (a0^2 + a1^2).
template <class P>
struct F64x2 {
  typedef F64<P> F;
  static constexpr int WORDS = 2 * P::N;
  F c0, c1;
  static F64x2 zero() { F64x2 r; r.c0 = F::zero(); r.c1 = F::zero(); return r; }
  static F64x2 one() { F64x2 r; r.c0 = F::one(); r.c1 = F::zero(); return r; }
  static F64x2 load(const uint32_t* p) { F64x2 r; r.c0 = F::load(p); r.c1 = F::load(p + P::N); return r; }
  void store(uint32_t* p) const { c0.store(p); c1.store(p + P::N); }
  bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  F64x2 add(const F64x2& o) const { F64x2 r; r.c0 = c0.add(o.c0); r.c1 = c1.add(o.c1); return r; }
  F64x2 sub(const F64x2& o) const { F64x2 r; r.c0 = c0.sub(o.c0); r.c1 = c1.sub(o.c1); return r; }
  F64x2 dbl() const { return add(*this); }
  F64x2 mul(const F64x2& o) const {      // Karatsuba: 3 products
    const F v0 = c0.mul(o.c0), v1 = c1.mul(o.c1);
    F64x2 r; r.c0 = v0.sub(v1); r.c1 = c0.add(c1).mul(o.c0.add(o.c1)).sub(v0).sub(v1);
    return r;
  }
  F64x2 sqr() const { F64x2 r; r.c0 = c0.add(c1).mul(c0.sub(c1)); r.c1 = c0.dbl().mul(c1); return r; }
  F64x2 inv() const {
    const F ni = c0.sqr().add(c1.sqr()).inv();
    F64x2 r; r.c0 = c0.mul(ni); r.c1 = F::zero().sub(c1).mul(ni);
    return r;
  }
};

}  // namespace host64
template <class C1> struct G2Of;      // ec.hpp
template <class T> struct TeOf;       // ec.hpp; its host point, Xyzz64<TeOf<T>>, is in te.hpp
template <class C> struct AffD;
template <class C> struct XyzzD;
namespace host64 {
template <class C> struct Coord64Of { typedef F64<typename C::FqP> type; };
template <class C> struct IsTe { static constexpr bool value = false; };
template <class T> struct IsTe<TeOf<T>> { static constexpr bool value = true; };
template <class C1> struct Coord64Of<G2Of<C1>> { typedef F64x2<typename C1::FqP> type; };

template <class C>
struct Xyzz64 {
  typedef typename Coord64Of<C>::type Fq;
  static constexpr int FW = Fq::WORDS;   // 32-bit words per coordinate
  Fq X, Y, ZZ, ZZZ;
  static Xyzz64 infinity() { Xyzz64 r; r.X = r.Y = r.ZZ = r.ZZZ = Fq::zero(); return r; }
  bool is_inf() const { return ZZ.is_zero(); }
  void store(uint32_t* p) const { X.store(p); Y.store(p + FW); ZZ.store(p + 2 * FW); ZZZ.store(p + 3 * FW); }
  static Xyzz64 load(const uint32_t* p) { Xyzz64 r; r.X = Fq::load(p); r.Y = Fq::load(p + FW); r.ZZ = Fq::load(p + 2 * FW); r.ZZZ = Fq::load(p + 3 * FW); return r; }
  // an affine point x||y (2 * FW words; all zero: infinity)
  static Xyzz64 from_affine(const uint32_t* xy) {
    bool inf = true; for (int i = 0; i < 2 * FW; i++) inf &= xy[i] == 0;
    if (inf) return infinity();
    Xyzz64 r; r.X = Fq::load(xy); r.Y = Fq::load(xy + FW); r.ZZ = r.ZZZ = Fq::one();
    return r;
  }
  Xyzz64 dbl() const {   // dbl-2008-s-1, a = 0
    if (is_inf() || Y.is_zero()) return infinity();
    Xyzz64 r;
    Fq U = Y.dbl(), V = U.sqr(), W = U.mul(V), S = X.mul(V), xx = X.sqr(), M = xx.dbl().add(xx);
    r.X = M.sqr().sub(S.dbl());
    r.Y = M.mul(S.sub(r.X)).sub(W.mul(Y));
    r.ZZ = V.mul(ZZ); r.ZZZ = W.mul(ZZZ);
    return r;
  }
  void add(const Xyzz64& o) {   // add-2008-s
    if (o.is_inf()) return;
    if (is_inf()) { *this = o; return; }
    Fq U1 = X.mul(o.ZZ), U2 = o.X.mul(ZZ), S1 = Y.mul(o.ZZZ), S2 = o.Y.mul(ZZZ);
    Fq Pp = U2.sub(U1), R = S2.sub(S1);
    if (Pp.is_zero()) { if (R.is_zero()) *this = dbl(); else *this = infinity(); return; }
    Fq PP = Pp.sqr(), PPP = Pp.mul(PP), Q = U1.mul(PP);
    Fq X3 = R.sqr().sub(PPP).sub(Q.dbl());
    Y = R.mul(Q.sub(X3)).sub(S1.mul(PPP));
    X = X3;
    ZZ = ZZ.mul(o.ZZ).mul(PP); ZZZ = ZZZ.mul(o.ZZZ).mul(PPP);
  }
  // affine x||y (Montgomery); (0,0) for infinity
  void store_affine(uint32_t* out) const {
    if (is_inf()) { memset(out, 0, 2 * FW * 4); return; }
    Fq t = ZZ.mul(ZZZ).inv();
    X.mul(t.mul(ZZZ)).store(out); Y.mul(t.mul(ZZ)).store(out + FW);
  }
};

// out = k * pt for an affine point pt, as an affine point: double-and-add from the top bit of the canonical scalar (G::FrP::N words)
template <class G>
void scalar_mul(const uint32_t* pt, const uint32_t* k_canonical, uint32_t* out_affine) {
  const Xyzz64<G> base = Xyzz64<G>::from_affine(pt);
  Xyzz64<G> acc = Xyzz64<G>::infinity();
  for (int bit = G::FrP::N * 32 - 1; bit >= 0; bit--) {
    acc = acc.dbl();
    if ((k_canonical[bit >> 5] >> (bit & 31)) & 1) acc.add(base);
  }
  acc.store_affine(out_affine);
}

// out = the sum of `count` affine points of G as an affine point (the group law of the device code, ec.hpp, run on the host)
template <class G>
void points_sum(const uint32_t* pts, size_t count, uint32_t* out_affine) {
  if constexpr (IsTe<G>::value) { Xyzz64<G>::points_sum(pts, count, out_affine); return; }      // (the caller's points are x || y, the device's affine form is not)
  else {
  XyzzD<G> acc = XyzzD<G>::infinity();
  for (size_t i = 0; i < count; i++) acc.add_affine(AffD<G>::load(pts + i * AffD<G>::WORDS));
  acc.to_affine().store(out_affine);
  }
}

struct WeightedPoint { uint32_t exponent; const uint32_t* xyzz; };

// out = sum_i 2^exponent_i * P_i as an affine point: one descending Horner chain.
template <class C>
void horner_to_affine(std::vector<WeightedPoint>& items, uint32_t* out_affine) {
  std::stable_sort(items.begin(), items.end(), [](const WeightedPoint& a, const WeightedPoint& b) { return a.exponent > b.exponent; });
  Xyzz64<C> acc = Xyzz64<C>::infinity();
  uint32_t cur = items.empty() ? 0 : items[0].exponent;
  for (const auto& it : items) {
    for (; cur > it.exponent; cur--) acc = acc.dbl();
    acc.add(Xyzz64<C>::load(it.xyzz));
  }
  for (; cur > 0; cur--) acc = acc.dbl();
  acc.store_affine(out_affine);
}

// count XYZZ points -> count affine points (x||y Montgomery, (0,0) = infinity) with ONE field
// inversion (Montgomery's trick over the products ZZ*ZZZ).
template <class C>
void batch_to_affine(const uint32_t* xyzz, size_t count, uint32_t* out_affine) {
  if constexpr (IsTe<C>::value) { Xyzz64<C>::batch_to_affine(xyzz, count, out_affine); return; }
  else {
  typedef Xyzz64<C> P; typedef typename P::Fq Fq;
  constexpr int FW = P::FW;
  std::vector<Fq> prefix(count);
  Fq run = Fq::one();
  for (size_t i = 0; i < count; i++) {
    P p = P::load(xyzz + i * 4 * FW);
    prefix[i] = run;
    if (!p.is_inf()) run = run.mul(p.ZZ.mul(p.ZZZ));
  }
  Fq inv = run.inv();
  for (size_t i = count; i-- > 0;) {
    P p = P::load(xyzz + i * 4 * FW);
    uint32_t* o = out_affine + i * 2 * FW;
    if (p.is_inf()) { memset(o, 0, 2 * FW * 4); continue; }
    Fq t = inv.mul(prefix[i]);                 // 1 / (ZZ * ZZZ) of point i
    inv = inv.mul(p.ZZ.mul(p.ZZZ));
    p.X.mul(t.mul(p.ZZZ)).store(o); p.Y.mul(t.mul(p.ZZ)).store(o + FW);
  }
  }
}

// Window table of one fixed base (affine, 2 * FW words; all zero: infinity) for signed radix-2^c digits:
//   tbl[w * 2^(c-1) + d - 1] = d * 2^(c w) * base,  d = 1 .. 2^(c-1),  w < Wd      (affine, one inversion for all of it)
// what FixedBaseTableMulBody (ipa.hpp) reads; G is a curve or G2Of<curve>.
template <class G>
void fixed_base_window_table(const uint32_t* base, uint32_t c, uint32_t Wd, std::vector<uint32_t>& tbl) {
  typedef Xyzz64<G> P;
  constexpr int FW = P::FW;
  const uint32_t half = 1u << (c - 1);
  std::vector<uint32_t> xyzz((size_t)Wd * half * 4 * FW);
  tbl.assign((size_t)Wd * half * 2 * FW, 0);
  P b = P::from_affine(base);
  for (uint32_t w = 0; w < Wd; w++) {
    P cur = b;
    for (uint32_t d = 0; d < half; d++) { cur.store(&xyzz[((size_t)w * half + d) * 4 * FW]); cur.add(b); }
    for (uint32_t k = 0; k < c; k++) b = b.dbl();
  }
  batch_to_affine<G>(xyzz.data(), (size_t)Wd * half, tbl.data());
}

}  // namespace host64
}  // namespace pc
