// TEST-ONLY host driver for the radix-2^30 field and running sum (poly_commit_amd/csrc/fp30.hpp, ec.hpp XyzzR30): raw limbs in and
// out for tests/test_fq30_cpu.py, which checks them against Python integers.  With -DFQ30_SELFTEST_MAIN it is a program of its own
// (the sanitizer build: random chains of additions against XyzzD::add_affine_lz).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../poly_commit_amd/csrc/ec.hpp"

typedef pc::Fq30 F;
typedef pc_curve_bls12_381 C;
typedef pc::Fd<C::FqP> F32;
typedef pc::XyzzD<C> Pt32;
typedef pc::AffD<C> Aff;

static F ld(const uint32_t* p) { F r; for (int i = 0; i < 13; i++) r.l[i] = p[i]; return r; }
static void st(const F& a, uint32_t* p) { for (int i = 0; i < 13; i++) p[i] = a.l[i]; }

// limbs 0..11 below 2^30 and value <= V p
static bool in_class(const F& a, int V) {
  for (int i = 0; i < 12; i++) if (a.l[i] >> 30) return false;
  const F::L13 k = F::kp(V);
  for (int i = 12; i >= 0; i--) { if (a.l[i] < k.v[i]) return true; if (a.l[i] > k.v[i]) return false; }
  return true;
}

extern "C" int fq30_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
  switch (op) {
    case 0: st(F::mul<64, 2>(ld(a), ld(b)), out); break;
    case 1: st(F::sqr<66>(ld(a)), out); break;
    case 2: st(F::mul_add_mul<66, 16, 64, 2>(ld(a), ld(b), ld(c), ld(d)), out); break;
    case 3: st(F::sub<64>(ld(a), ld(b)), out); break;
    case 4: st(F::sub_dbl<4>(ld(a), ld(b)), out); break;
    case 5: st(F::neg<64>(ld(a)), out); break;
    case 6: st(F::from32(F32::load(a)), out); break;
    case 7: ld(a).to32().store(out); break;
    case 8: out[0] = ld(a).is_zero_modp<66>() ? 1 : 0; break;
    case 9: st(ld(a).reduce(), out); break;
    case 10: st(F::one(), out); break;
    case 11: st(F::sub<2>(ld(a), ld(b)), out); break;
    case 12: st(F::sub<14>(ld(a), ld(b)), out); break;
    case 13: st(F::mul<66, 8>(ld(a), ld(b)), out); break;
    case 14: out[0] = ld(a).is_zero_exact() ? 1 : 0; break;
    default: return 1;
  }
  return 0;
}

// the column plan of one multiplier form: split[25][3] as bytes; returns Plan::ok
extern "C" int fq30_plan(int kind, int va, int vb, int vc, int vd, uint8_t* split) {
  const F::Plan pl = F::plan(kind, va, vb, vc, vd);
  for (int k = 0; k < 25; k++) for (int g = 0; g < 3; g++) split[3 * k + g] = pl.split[k][g];
  return pl.ok ? 1 : 0;
}

// table of 64 affine points: entry 0 = infinity (0, 0), entry k = k G
static void make_table(Aff* tbl) {
  Aff g; for (int i = 0; i < 12; i++) { g.x.l[i] = C::GX[i]; g.y.l[i] = C::GY[i]; }
  tbl[0] = Aff::infinity();
  Pt32 acc = Pt32::from_affine(g);
  for (int k = 1; k < 64; k++) { tbl[k] = acc.to_affine(); acc.add_affine(g); }
}

// A chain of additions from infinity: idx[i] = table entry | sign << 31.  Three running sums: radix 2^30, lazily reduced radix 2^32,
// canonical; each handed back canonical (4 x 12 words).  Returns the number of steps after which the radix-2^30 sum broke its
// invariant (X, Y of class 64, ZZ, ZZZ of class 2) or differed from the lazily reduced one.
extern "C" int fq30_chain(size_t n, const uint32_t* idx, uint32_t* out_r30, uint32_t* out_lz, uint32_t* out_canon) {
  Aff tbl[64];
  make_table(tbl);
  pc::XyzzR30 a30 = pc::XyzzR30::infinity();
  Pt32 alz = Pt32::infinity(), ac = Pt32::infinity();
  int bad = 0;
  for (size_t i = 0; i < n; i++) {
    const Aff& pt = tbl[idx[i] & 63];
    const bool neg = (idx[i] >> 31) != 0;
    a30.add_affine(pt, neg);
    alz.add_affine_lz(pt, neg);
    ac.add_affine(pt.neg_if(neg));
    bool ok = in_class(a30.X, 64) && in_class(a30.Y, 64) && in_class(a30.ZZ, 2) && in_class(a30.ZZZ, 2);
    const Pt32 c30 = a30.to32().canonical(), clz = alz.canonical();
    uint32_t w30[48], wlz[48];
    c30.store(w30); clz.store(wlz);
    ok = ok && (c30.is_inf() ? clz.is_inf() : memcmp(w30, wlz, sizeof w30) == 0) && c30.is_inf() == a30.is_inf();
    bad += !ok;
  }
  a30.to32().canonical().store(out_r30);
  alz.canonical().store(out_lz);
  ac.store(out_canon);
  return bad;
}

#ifdef FQ30_SELFTEST_MAIN
int main() {
  uint32_t idx[4000];
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 4000; i++) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    idx[i] = (uint32_t)(s >> 33) & 63;
    if ((s >> 20) & 1) idx[i] |= 1u << 31;
  }
  // special cases: doubling from a fresh sum, P + (-P), an infinite base
  idx[0] = 5; idx[1] = 5; idx[2] = 0; idx[3] = 10 | (1u << 31);
  uint32_t o30[48], olz[48], oc[48];
  const int bad = fq30_chain(4000, idx, o30, olz, oc);
  const Pt32 pc_ = Pt32::load(oc), p30 = Pt32::load(o30);
  const Aff ac = pc_.to_affine(), a30 = p30.to_affine();
  const bool same = ac.x.eq(a30.x) && ac.y.eq(a30.y);
  printf("fq30 selftest: %d bad steps, affine sums %s\n", bad, same ? "equal" : "DIFFER");
  return bad != 0 || !same;
}
#endif
