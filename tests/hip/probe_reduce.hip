// TEST-ONLY probe unit: the MSM's bucket reduction on its own, for tests/test_msm_reduce_gpu.py and tests/test_msm_reduce_cpu.py
// (tests/harness/reduceref.py).  The device build owns a pc::HipBackend and calls HipBackend::bucket_level -- the serial
// BucketLevelBody, k_bucket_level_coop or k_bucket_level_coop2 of csrc/msm_coop.hpp -- level by level; the host build steps
// BucketLevelBody (mode 0) and BucketLevelBitsBody (modes 1 and 2) lane by lane, which is what the backends of tests/emu do.  A call's
// geometry comes from msm_make_geom and its level plan from msm_plan_levels, the builders MsmPlan::plan_geometry uses, under the
// configuration the product gives the group (G2: K1 = 128 and no two-lane levels, csrc/abi_g2.hip and csrc/blocking_lane.hpp).
// Host pointers in and out, the HIP status is the return value (0 in the host build).
//
// group: 0 BLS12-381, 1 BN254, 2 Pallas, 3 BLS12-377 (G1), 4 G2 of BLS12-381.  Points are XYZZ words (4 coordinates, Montgomery form).
// knobs[6]: K0, tbl_K0, K1, coop_max_points, coop2_max_points, coop2_max_entries; 0 keeps the default, all ones (2^64 - 1) sets 0.
// PROBE_BAD_OP, before anything is allocated or launched, for: K no power of two or below 2; modes 1 and 2 with K < 16 or K > 256;
// mode 2 with K > 128; mode 2 or K > 128 on G2 (the product throws there); cnt (1 + n_old) = 0; more than 2^21 input points; an
// output buffer shorter than the level's arrays and the cnt points behind them; a geometry msm_make_geom or MsmPlan would refuse.
#include "probe_runner.hpp"
#include <string.h>
#include <stdlib.h>

enum { REDUCE_PLAN_WORDS = 200, REDUCE_MAX_POINTS = 1 << 21 };

#if defined(__HIPCC__)
#include "../../poly_commit_amd/csrc/hip_backend_msm.hpp"
#else
#include "../../poly_commit_amd/csrc/msm.hpp"
#include "../../poly_commit_amd/csrc/g2.hpp"
#endif

namespace probe_reduce {

#if defined(__HIPCC__)
// the device side: the unit's own pc::HipBackend; blocking copies, as the other probe units make them
struct Be {
  pc::HipBackend* b = nullptr;
  void open() {
    static pc::HipBackend* be = nullptr;
    if (!be) { pc::HipBackend* n = new pc::HipBackend(); n->init(); be = n; }
    b = be;
  }
  void* alloc(size_t bytes) { return b->alloc(bytes); }
  void free(void* p) { if (b) b->free(p); }
  void fill(void* p, int v, size_t bytes) { b->memset(p, v, bytes); }
  void h2d(void* d, const void* s, size_t bytes) { if (bytes) PC_HIP_CHECK(hipMemcpy(d, s, bytes, hipMemcpyHostToDevice)); }
  void d2h(void* d, const void* s, size_t bytes) { b->sync(); if (bytes) PC_HIP_CHECK(hipMemcpy(d, s, bytes, hipMemcpyDeviceToHost)); }
  void quiet() { if (b) (void)hipStreamSynchronize(b->stream); }
  template <class C>
  void level(uint32_t K, uint32_t woff, uint32_t cnt, uint32_t n_old, int mode, const uint32_t* x, const uint32_t* old_in, uint32_t* out) {
    b->template bucket_level<C>(K, woff, cnt, n_old, mode, x, old_in, out);
  }
  template <class B> void launch(const B& body, size_t lanes) { b->launch(body, lanes); }
};
template <class F> static int guarded(F f) {
  try { f(); } catch (const pc::HipError& e) { return (int)e.code; } catch (...) { return (int)hipErrorUnknown; }
  return 0;
}
#else
// the host side: every body a plain loop over its lanes
struct Be {
  void open() {}
  void* alloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
  void free(void* p) { if (p) ::free(p); }
  void fill(void* p, int v, size_t bytes) { memset(p, v, bytes); }
  void h2d(void* d, const void* s, size_t bytes) { if (bytes) memcpy(d, s, bytes); }
  void d2h(void* d, const void* s, size_t bytes) { if (bytes) memcpy(d, s, bytes); }
  void quiet() {}
  template <class C>
  void level(uint32_t K, uint32_t woff, uint32_t cnt, uint32_t n_old, int mode, const uint32_t* x, const uint32_t* old_in, uint32_t* out) {
    if (mode) {
      uint32_t lgK = 0; while ((1u << lgK) < K) lgK++;
      pc::BucketLevelBitsBody<C> b{K, lgK, woff, cnt, n_old, x, old_in, out};
      launch(b, (size_t)cnt * (1 + n_old));
    } else {
      pc::BucketLevelBody<C> b{K, woff, cnt, n_old, x, old_in, out};
      launch(b, (size_t)cnt * (1 + n_old));
    }
  }
  template <class B> void launch(const B& body, size_t lanes) { for (size_t i = 0; i < lanes; i++) body((uint32_t)i); }
};
template <class F> static int guarded(F f) {
  try { f(); } catch (...) { return 1; }
  return 0;
}
#endif

template <class C> struct IsG2 { static constexpr bool value = pc::ScalarCurveOf<C>::IS_G2; };

// what one level may be asked to do (HipBackend::bucket_level's preconditions, and the kernels' launch shapes)
template <class C>
static bool level_ok(uint32_t K, uint32_t woff, uint64_t cnt, uint32_t n_old, int mode) {
  if (K < 2 || (K & (K - 1)) || woff > 1 || mode < 0 || mode > 2 || n_old > 31) return false;
  if (mode && (K < 16 || K > 256)) return false;
  if (mode == 2 && K > 128) return false;
  if (IsG2<C>::value && (mode == 2 || K > 128)) return false;
  if (cnt * (1 + n_old) == 0 || cnt > REDUCE_MAX_POINTS) return false;
  if (cnt * K * (1 + n_old) > REDUCE_MAX_POINTS) return false;
  return true;
}

static uint32_t arrays_of(uint32_t K, uint32_t woff, uint32_t n_old, int mode) {      // the level's arrays, S included
  uint32_t lgK = 0; while ((1u << lgK) < K) lgK++;
  return 1 + (mode ? lgK + woff : 1u) + n_old;
}

struct Planned { pc::MsmGeom g; pc::MsmLevels lv; };

// geometry and level plan of a call, as MsmPlan makes them: the group's configuration, the knobs, the constructor's clamps
template <class C>
static bool make_plan(size_t n, uint32_t c, uint32_t tbl, uint32_t glv, uint32_t subs, const uint64_t* knobs, Planned* out) {
  typedef typename C::FrP FrP;
  if (n == 0 || n > 0xffffffffull || c < 2 || c > 24 || tbl > 1 || glv > 1) return false;
  if ((glv || subs) && !tbl) return false;                      // both are table modes
  if (IsG2<C>::value && tbl) return false;                      // MsmPlan: G2 is table-free
  if (glv && !pc::HasGlv<C>::value) return false;
  if (subs && n % subs) return false;
  pc::MsmConfig cfg;
  if (IsG2<C>::value) { cfg.K1 = 128; cfg.coop2_max_points = 0; }
  auto knob = [&](int i, uint64_t dflt) { return knobs[i] == 0 ? dflt : knobs[i] == ~0ull ? 0ull : knobs[i]; };
  for (int i = 0; i < 5; i++) if (knob(i, 0) > 0xffffffffull) return false;
  cfg.K0 = (uint32_t)knob(0, cfg.K0); cfg.tbl_K0 = (uint32_t)knob(1, cfg.tbl_K0); cfg.K1 = (uint32_t)knob(2, cfg.K1);
  cfg.coop_max_points = (uint32_t)knob(3, cfg.coop_max_points); cfg.coop2_max_points = (uint32_t)knob(4, cfg.coop2_max_points);
  cfg.coop2_max_entries = (size_t)knob(5, cfg.coop2_max_entries);
  auto pow2_floor = [](uint32_t v, uint32_t lo, uint32_t hi) { uint32_t p = lo; while (p * 2 <= v && p * 2 <= hi) p *= 2; return p; };
  cfg.K0 = pow2_floor(cfg.K0, 2, 1u << 12);
  cfg.tbl_K0 = pow2_floor(cfg.tbl_K0, 2, 1u << 12);
  cfg.K1 = pow2_floor(cfg.K1, 2, 256);
  out->g = pc::msm_make_geom(FrP::BITS, n, c, tbl != 0, glv != 0, subs, tbl ? (uint32_t)(subs ? n / subs : n) : 0u, 0u, cfg.T2, cfg.T2b);
  if ((uint64_t)out->g.W * out->g.nb_win > 0xfffffffeull) return false;
  out->lv = pc::msm_plan_levels(cfg, out->g, n, tbl != 0);
  return out->lv.n_levels <= 32 && out->lv.arr_exp.size() <= 64;
}

template <class C>
static int plan(size_t n, uint32_t c, uint32_t tbl, uint32_t glv, uint32_t subs, const uint64_t* knobs, uint32_t* out) {
  Planned p;
  if (!make_plan<C>(n, c, tbl, glv, subs, knobs, &p)) return PROBE_BAD_OP;
  memset(out, 0, REDUCE_PLAN_WORDS * 4);
  out[0] = p.g.W; out[1] = p.g.Wd; out[2] = p.g.nb_win; out[3] = p.lv.n_levels;
  for (uint32_t l = 0; l < p.lv.n_levels; l++) { uint32_t* o = out + 4 + 4 * l; o[0] = p.lv.K[l]; o[1] = p.lv.mode[l]; o[2] = p.lv.m[l]; o[3] = p.lv.narr[l]; }
  out[132] = (uint32_t)p.lv.arr_exp.size();
  for (size_t a = 0; a < p.lv.arr_exp.size(); a++) out[133 + a] = p.lv.arr_exp[a];
  return 0;
}

template <class C>
static int level(uint32_t K, uint32_t woff, uint32_t cnt, uint32_t n_old, int mode, const uint32_t* x, const uint32_t* old_in, uint32_t* out,
                 size_t out_points) {
  constexpr size_t PW = pc::XyzzD<C>::WORDS;
  if (!level_ok<C>(K, woff, cnt, n_old, mode)) return PROBE_BAD_OP;
  const size_t need = (size_t)cnt * arrays_of(K, woff, n_old, mode) + cnt;
  if (out_points < need || out_points > 2 * (size_t)REDUCE_MAX_POINTS) return PROBE_BAD_OP;
  const size_t in_pts = (size_t)cnt * K;
  Be be;
  uint32_t *dx = nullptr, *dold = nullptr, *dout = nullptr;
  const int st = guarded([&]() {
    be.open();
    dx = (uint32_t*)be.alloc(in_pts * PW * 4); dold = (uint32_t*)be.alloc(in_pts * n_old * PW * 4); dout = (uint32_t*)be.alloc(out_points * PW * 4);
    be.h2d(dx, x, in_pts * PW * 4); be.h2d(dold, old_in, in_pts * n_old * PW * 4);
    be.fill(dout, 0xff, out_points * PW * 4);                     // what the level does not write stays recognisable
    be.template level<C>(K, woff, cnt, n_old, mode, dx, n_old ? dold : nullptr, dout);
    be.d2h(out, dout, out_points * PW * 4);
  });
  be.quiet();
  be.free(dx); be.free(dold); be.free(dout);
  return st;
}

// every level of the plan over `buckets` (W x nb_win points), in the layout of MsmPlan::reduce_and_download: per level
// [S][new arrays][older arrays], each W x m points; out_arrays: the arrays behind S of the last level (W points each);
// out_fold (subs != 0): what SubFoldBody makes of them, W points
template <class C>
static int all(size_t n, uint32_t c, uint32_t tbl, uint32_t glv, uint32_t subs, const uint64_t* knobs, const uint32_t* buckets,
               uint32_t* out_arrays, uint32_t* out_fold) {
  typedef pc::XyzzD<C> Pt;
  constexpr size_t PW = Pt::WORDS;
  Planned p;
  if (!make_plan<C>(n, c, tbl, glv, subs, knobs, &p)) return PROBE_BAD_OP;
  const pc::MsmGeom& g = p.g; const pc::MsmLevels& lv = p.lv;
  const size_t NB = (size_t)g.W * g.nb_win;
  if (lv.n_levels == 0 || NB > REDUCE_MAX_POINTS || lv.arr_exp.size() > 32) return PROBE_BAD_OP;
  size_t red_points = 0;
  for (uint32_t l = 0; l < lv.n_levels; l++) {
    const uint32_t n_old = l ? lv.narr[l - 1] : 0;
    if (!level_ok<C>(lv.K[l], l == 0 ? 1u : 0u, (uint64_t)g.W * lv.m[l], n_old, (int)lv.mode[l])) return PROBE_BAD_OP;
    if (arrays_of(lv.K[l], l == 0 ? 1u : 0u, n_old, (int)lv.mode[l]) != 1 + lv.narr[l]) return PROBE_BAD_OP;
    red_points += (size_t)(1 + lv.narr[l]) * g.W * lv.m[l];
  }
  if (red_points > 4 * (size_t)REDUCE_MAX_POINTS) return PROBE_BAD_OP;
  Be be;
  uint32_t *dbuckets = nullptr, *red = nullptr;
  const int st = guarded([&]() {
    be.open();
    dbuckets = (uint32_t*)be.alloc(NB * PW * 4); red = (uint32_t*)be.alloc((red_points + g.W) * PW * 4);
    be.h2d(dbuckets, buckets, NB * PW * 4);
    be.fill(red, 0xff, (red_points + g.W) * PW * 4);
    const uint32_t* x = dbuckets;
    uint32_t* lvl_base = red;
    uint32_t* prev_base = nullptr;
    for (uint32_t l = 0; l < lv.n_levels; l++) {
      const size_t cnt = (size_t)g.W * lv.m[l];
      const uint32_t n_old = l ? lv.narr[l - 1] : 0;
      const uint32_t* old_in = l ? prev_base + (size_t)g.W * lv.m[l - 1] * PW : nullptr;
      be.template level<C>(lv.K[l], l == 0 ? 1u : 0u, (uint32_t)cnt, n_old, (int)lv.mode[l], x, old_in, lvl_base);
      x = lvl_base; prev_base = lvl_base; lvl_base += (size_t)(1 + lv.narr[l]) * cnt * PW;
    }
    const uint32_t* arrays = prev_base + (size_t)g.W * PW;
    if (subs) {
      pc::SubFoldBody<C> f;
      f.arrays = arrays; f.W = g.W; f.narr = (uint32_t)lv.arr_exp.size();
      for (uint32_t a = 0; a < f.narr; a++) { f.exp[a] = lv.arr_exp[a]; f.order[a] = a; }
      for (uint32_t a = f.narr; a < 32; a++) { f.exp[a] = 0; f.order[a] = 0; }
      std::stable_sort(f.order, f.order + f.narr, [&](uint32_t a, uint32_t b) { return f.exp[a] > f.exp[b]; });
      f.out = red + red_points * PW;
      be.launch(f, g.W);
      be.d2h(out_fold, f.out, (size_t)g.W * PW * 4);
    }
    be.d2h(out_arrays, arrays, (size_t)g.W * lv.narr[lv.n_levels - 1] * PW * 4);
  });
  be.quiet();
  be.free(dbuckets); be.free(red);
  return st;
}

}  // namespace probe_reduce

#define REDUCE_DISPATCH(fn, ...)                                                  \
  switch (group) {                                                                \
    case 0: return probe_reduce::fn<pc_curve_bls12_381>(__VA_ARGS__);             \
    case 1: return probe_reduce::fn<pc_curve_bn254>(__VA_ARGS__);                 \
    case 2: return probe_reduce::fn<pc_curve_pallas>(__VA_ARGS__);                \
    case 3: return probe_reduce::fn<pc_curve_bls12_377>(__VA_ARGS__);             \
    case 4: return probe_reduce::fn<pc::G2Of<pc_curve_bls12_381>>(__VA_ARGS__);   \
    default: return PROBE_BAD_OP;                                                 \
  }

// out (REDUCE_PLAN_WORDS words): W | Wd | nb_win | levels | 32 x (K, mode, m, narr) | number of exponents | arr_exp (up to 64)
extern "C" int pc_probe_reduce_plan(int group, size_t n, uint32_t c, uint32_t tbl, uint32_t glv, uint32_t subs, const uint64_t* knobs,
                                    uint32_t* out) {
  REDUCE_DISPATCH(plan, n, c, tbl, glv, subs, knobs, out)
}

// x: cnt x K points; old_in: n_old x cnt x K points; out: out_points >= cnt (arrays + 1) points, preset to 0xff bytes
extern "C" int pc_probe_reduce_level(int group, uint32_t K, uint32_t weight_off, uint32_t cnt, uint32_t n_old, int mode, const uint32_t* x,
                                     const uint32_t* old_in, uint32_t* out, size_t out_points) {
  REDUCE_DISPATCH(level, K, weight_off, cnt, n_old, mode, x, old_in, out, out_points)
}

// buckets: W x nb_win points; out_arrays: narr x W points; out_fold: W points, written when subs != 0
extern "C" int pc_probe_reduce_all(int group, size_t n, uint32_t c, uint32_t tbl, uint32_t glv, uint32_t subs, const uint64_t* knobs,
                                   const uint32_t* buckets, uint32_t* out_arrays, uint32_t* out_fold) {
  REDUCE_DISPATCH(all, n, c, tbl, glv, subs, knobs, buckets, out_arrays, out_fold)
}
