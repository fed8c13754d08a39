// TEST-ONLY probe unit: the MSM's bucket sort on its own (HipBackend::sort_entries, csrc/hip_backend_msm.hpp: the LDS radix sort of
// csrc/msm_sort.hpp or sort_entries_atomic of csrc/msm.hpp), for tests/test_msm_sort_gpu.py (tests/harness/sortref.py).  The unit owns a
// pc::HipBackend; a call's MsmGeom comes from msm_make_geom, the builder MsmPlan::plan_geometry uses, and gets its per-call fields the
// way MsmPlan::part_body sets them; the sort's own geometry and its choice of path come from make_sort_geom, sort_needs_atomic and
// sort_pass_threads.  Host pointers in and out, the HIP status is the return value.  The host build has the entry points and
// answers PROBE_UNSUPPORTED: the sort is device code only.
//
// A call is described by (curve, n, c, W, Wd, tbl_stride, m_sub, glv):
//   tbl_stride == 0             table-free: one bucket set per window
//   tbl_stride != 0             against a window table of tbl_stride points per window: one shared bucket set, two with glv
//   m_sub != 0                  n / m_sub independent MSMs of m_sub pairs over the table, one bucket set (pair) each
// W and Wd are what the caller expects the builder to derive; a call whose W or Wd differ from the builder's, or that leaves the
// documented preconditions (2 <= c <= 24, Wd c > 32 (N - 1), base indices below 2^31, n Wd entries countable in 32 bits), is
// refused with PROBE_BAD_OP before anything is allocated or launched.
#include "probe_runner.hpp"

enum { SORT_GEOM_WORDS = 16 };

#if defined(__HIPCC__)
#include "../../poly_commit_amd/csrc/hip_backend_msm.hpp"

namespace probe_sort {

template <class C>
static bool make_geom(size_t n, uint32_t c, uint32_t W, uint32_t Wd, uint32_t tbl_stride, uint32_t m_sub, uint32_t glv, uint32_t base_off,
                      pc::MsmGeom* out) {
  typedef typename C::FrP FrP;
  if (n == 0 || n > 0xffffffffull || c < 2 || c > 24 || glv > 1) return false;
  if ((glv || m_sub) && !tbl_stride) return false;                      // both are table modes
  if (glv && !pc::HasGlv<C>::value) return false;
  if (m_sub && n % m_sub) return false;
  const uint32_t subs = m_sub ? (uint32_t)(n / m_sub) : 0u;
  const pc::MsmGeom g = pc::msm_make_geom(FrP::BITS, n, c, tbl_stride != 0, glv != 0, subs, tbl_stride, 0u, 8u, 8u);
  if (g.W != W || g.Wd != Wd) return false;
  if ((uint64_t)g.windows() * c <= 32ull * ((glv ? 5 : FrP::N) - 1)) return false;
  const uint64_t per_msm = m_sub ? m_sub : n;
  if (tbl_stride && (uint64_t)base_off + per_msm > tbl_stride) return false;      // a window's row of the table holds the call's bases
  const uint64_t top_base = (uint64_t)(tbl_stride ? (g.windows() - 1) : 0u) * tbl_stride + base_off + per_msm - 1;
  if (top_base >= (1ull << 31)) return false;
  if ((uint64_t)n * g.Wd > 0xffffffffull || (uint64_t)g.W * g.nb_win > 0xfffffffeull) return false;
  *out = g;
  out->base_off = base_off; out->m_sub = m_sub;
  return true;
}

template <class C>
static int geom(size_t n, uint32_t c, uint32_t W, uint32_t Wd, uint32_t tbl_stride, uint32_t m_sub, uint32_t glv, uint32_t* out) {
  pc::MsmGeom g;
  if (!make_geom<C>(n, c, W, Wd, tbl_stride, m_sub, glv, 0, &g)) return PROBE_BAD_OP;
  const pc::SortGeom sg = pc::make_sort_geom(g, C::FrP::BITS);
  const uint32_t v[SORT_GEOM_WORDS] = {sg.cb, sg.fine_bits, sg.top_fine_bits, sg.NC, sg.nblocks, sg.S, (uint32_t)pc::sort_pass_lds_bytes(sg),
                                       (uint32_t)pc::sort_pass_threads(sg), pc::sort_needs_atomic(sg) ? 1u : 0u, g.W, g.Wd, g.nb_win, g.NB,
                                       sg.ncw, sg.top_w, 0u};
  for (int i = 0; i < SORT_GEOM_WORDS; i++) out[i] = v[i];
  return 0;
}

static pc::HipBackend* backend() {
  static pc::HipBackend* be = nullptr;
  if (!be) { pc::HipBackend* b = new pc::HipBackend(); b->init(); be = b; }
  return be;
}

template <class C>
static int sort(size_t n, uint32_t c, uint32_t W, uint32_t Wd, uint32_t tbl_stride, uint32_t m_sub, uint32_t glv, uint32_t from_mont,
                uint32_t base_off, int mode, int use_tab, const uint32_t* scalars, uint32_t* out_offsets, uint32_t* out_entries,
                uint32_t* out_path) {
  constexpr int FN = C::FrP::N;
  pc::MsmGeom g;
  if (!make_geom<C>(n, c, W, Wd, tbl_stride, m_sub, glv, base_off, &g) || from_mont > 1 || (mode != 0 && mode != 1)) return PROBE_BAD_OP;
  if (use_tab && !m_sub) return PROBE_BAD_OP;
  g.from_mont = from_mont;
  const size_t nb1 = (size_t)g.NB + 1, M = n * g.Wd, subs = m_sub ? n / m_sub : 0;
  uint32_t *d_sc = nullptr, *d_hist = nullptr, *d_off = nullptr, *d_cur = nullptr, *d_ent = nullptr;
  uint64_t* d_tab = nullptr;
  pc::HipBackend* be = nullptr;
  int st = 0;
  try {
    be = backend();
    d_sc = (uint32_t*)be->alloc(n * FN * 4); d_hist = (uint32_t*)be->alloc(nb1 * 4); d_off = (uint32_t*)be->alloc(nb1 * 4);
    d_cur = (uint32_t*)be->alloc(nb1 * 4); d_ent = (uint32_t*)be->alloc(M * 4);
    PC_HIP_CHECK(hipMemcpy(d_sc, scalars, n * FN * 4, hipMemcpyHostToDevice));      // (blocking copies, as the other probe units make them)
    be->memset(d_off, 0xff, nb1 * 4); be->memset(d_ent, 0xff, M * 4);       // what the sort does not write stays recognisable
    const uint32_t* sc_arg = d_sc;
    if (use_tab) {            // the scalar vectors through a table of their addresses, and no contiguous array at all
      std::vector<uint64_t> tab(subs);
      for (size_t s = 0; s < subs; s++) tab[s] = (uint64_t)(uintptr_t)(d_sc + s * m_sub * FN);
      d_tab = (uint64_t*)be->alloc(subs * 8);
      PC_HIP_CHECK(hipMemcpy(d_tab, tab.data(), subs * 8, hipMemcpyHostToDevice));
      g.scalar_tab = d_tab; sc_arg = nullptr;
    }
    be->sort_mode = mode == 1 ? 0 : -1;      // 0: the library's own choice (PC_HIP_SORT, then the geometry); 1: the atomic sort
    be->template sort_entries<C>(g, sc_arg, d_hist, d_off, d_cur, d_ent);
    *out_path = be->last_sort_atomic ? 1u : 0u;
    be->sync();
    PC_HIP_CHECK(hipMemcpy(out_offsets, d_off, nb1 * 4, hipMemcpyDeviceToHost));
    PC_HIP_CHECK(hipMemcpy(out_entries, d_ent, M * 4, hipMemcpyDeviceToHost));
  } catch (const pc::HipError& e) { st = (int)e.code; }
  catch (...) { st = (int)hipErrorUnknown; }
  if (be) {
    (void)hipStreamSynchronize(be->stream);
    void* ps[] = {d_sc, d_hist, d_off, d_cur, d_ent, d_tab};
    for (void* p : ps) be->free(p);
  }
  return st;
}

}  // namespace probe_sort

#define SORT_DISPATCH(fn, ...)                                       \
  switch (curve) {                                                   \
    case 0: return probe_sort::fn<pc_curve_bls12_381>(__VA_ARGS__);  \
    case 1: return probe_sort::fn<pc_curve_bn254>(__VA_ARGS__);      \
    case 2: return probe_sort::fn<pc_curve_pallas>(__VA_ARGS__);     \
    case 3: return probe_sort::fn<pc_curve_bls12_377>(__VA_ARGS__);  \
    default: return PROBE_BAD_OP;                                    \
  }
#else
#define SORT_DISPATCH(fn, ...) return (curve >= 0 && curve <= 3) ? PROBE_UNSUPPORTED : PROBE_BAD_OP;
#endif

// out: cb | fine_bits | top_fine_bits | NC | nblocks | S | LDS bytes of a coarse pass | its lanes | 1 if sort_entries takes the atomic
// sort | W | Wd | nb_win | NB | ncw | top_w | 0
extern "C" int pc_probe_sort_geom(int curve, size_t n, uint32_t c, uint32_t W, uint32_t Wd, uint32_t tbl_stride, uint32_t m_sub, uint32_t glv,
                                  uint32_t* out) {
  SORT_DISPATCH(geom, n, c, W, Wd, tbl_stride, m_sub, glv, out)
}

// scalars: n x N words; out_offsets: NB + 1 words; out_entries: n x Wd words (0xffffffff behind the offsets[NB] the sort wrote);
// mode: 0 as the library decides, 1 the atomic sort; use_tab: many-MSM mode reads its vectors through MsmGeom::scalar_tab;
// out_path: 0 the LDS sort ran, 1 the atomic sort
extern "C" int pc_probe_sort(int curve, size_t n, uint32_t c, uint32_t W, uint32_t Wd, uint32_t tbl_stride, uint32_t m_sub, uint32_t glv,
                             uint32_t from_mont, uint32_t base_off, int mode, int use_tab, const uint32_t* scalars, uint32_t* out_offsets,
                             uint32_t* out_entries, uint32_t* out_path) {
  SORT_DISPATCH(sort, n, c, W, Wd, tbl_stride, m_sub, glv, from_mont, base_off, mode, use_tab, scalars, out_offsets, out_entries, out_path)
}
