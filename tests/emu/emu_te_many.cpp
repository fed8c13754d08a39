// TEST-ONLY host compilation of the many-MSM pass over a twisted Edwards key: the window table of te.hpp (TeWindowRowBody,
// TeBatchAffineBody, te_window_table) and MsmPlan<TeOf<ed_on_bls12_381>> in its many-MSM mode (a bucket set per sub-MSM, SubFoldBody,
// one normalisation for all results), stepped lane by lane by a single-threaded backend and validated against tests/harness/teref.py
// on a machine without a GPU.  NOT part of the product library.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/msm.hpp"
#include "../../poly_commit_amd/csrc/te.hpp"

struct CpuStepBackend {
  void* alloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
  void free(void* p) { if (p) ::free(p); }
  void memset(void* p, int v, size_t bytes) { ::memset(p, v, bytes); }
  void mark() {}
  bool timing_marks(bool) { return true; }
  void aux_begin(int, int) {}
  int aux_end() { return -1; }
  void wait_token(int) {}
  int main_token() { return -1; }
  void record_done() {}
  void begin_tail() {}
  void end_tail() {}
  void quiesce() {}
  void wait_done() {}
  void* alloc_host(size_t b) { return calloc(1, b ? b : 1); }
  void free_host(void* p) { if (p) ::free(p); }
  void copy_d2h_async(void* d, const void* s, size_t bytes) { memcpy(d, s, bytes); }
  void sync() {}
  void copy_d2d(void* d, const void* s, size_t bytes) { memcpy(d, s, bytes); }
  void copy_h2d(void* d, const void* s, size_t bytes) { memcpy(d, s, bytes); }
  void exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n) {
    uint32_t acc = 0;
    for (size_t i = 0; i < n; i++) { uint32_t v = in[i]; out[i] = acc; acc += v; }
  }
  template <class C>
  void sort_entries(const pc::MsmGeom& g, const uint32_t* scalars, uint32_t* hist, uint32_t* offsets, uint32_t* cursor, uint32_t* entries) {
    pc::sort_entries_atomic<C>(*this, g, scalars, hist, offsets, cursor, entries);
  }
  template <class C>
  void accumulate(const pc::AccumulateBody<C>& body, size_t lanes) { launch(body, lanes); }
  template <class C>
  void seg_reduce_tail(const pc::MsmGeom& g, uint32_t level, uint32_t slots, uint32_t* const* pk, uint32_t* const* pp, int cur,
                       const uint32_t* offsets, uint32_t* buckets) {
    pc::seg_reduce_tail_serial<C>(*this, g, level, slots, pk, pp, cur, offsets, buckets);
  }
  template <class C>
  void bucket_level(uint32_t K, uint32_t weight_off, uint32_t cnt, uint32_t n_old, bool bits, const uint32_t* x, const uint32_t* old_in, uint32_t* out) {
    if (bits) {
      uint32_t lgK = 0; while ((1u << lgK) < K) lgK++;
      pc::BucketLevelBitsBody<C> b{K, lgK, weight_off, cnt, n_old, x, old_in, out};
      launch(b, (size_t)cnt * (1 + n_old));
    } else {
      pc::BucketLevelBody<C> b{K, weight_off, cnt, n_old, x, old_in, out};
      launch(b, (size_t)cnt * (1 + n_old));
    }
  }
  template <class B> void launch(const B& body, size_t lanes) { for (size_t i = 0; i < lanes; i++) body((uint32_t)i); }
};

typedef pc::TeOf<pc_te_ed_on_bls12_381> TeC;
typedef pc::XyzzD<TeC> Pt;
typedef pc::AffD<TeC> Aff;
typedef pc_ed_on_bls12_381_fr TeFrP;

// the width and the row count the library chooses for a table of m points
extern "C" void emu_te_many_shape(size_t m, uint32_t* out_c, uint32_t* out_Wd) {
  *out_c = pc::msm_choose_table_c(m, TeFrP::BITS, 0);
  *out_Wd = pc::msm_num_windows(TeFrP::BITS, *out_c);
}

// table[w][j] = 2^(c w) * bases[j], w < Wd, j < m: bases and table in the resident form (24 words a record), K points per inversion
extern "C" void emu_te_window_table(const uint32_t* bases, size_t m, uint32_t c, uint32_t Wd, uint32_t K, uint32_t* table) {
  std::vector<uint32_t> ext(m * Pt::WORDS + 1), scratch(m * Pt::Fq::N + 1);
  CpuStepBackend be;
  pc::te_window_table<TeC>(be, bases, m, c, Wd, table, ext.data(), scratch.data(), K);
}

// B MSMs of m pairs over bases[base_off .. base_off + m) in one pass: the table, then MsmPlan with subs = B.  scalars: B x m x 8 words,
// out: B x 16 words (x || y).  c == 0: the library's width.  empty != 0: the call is made with no pairs at all (MsmPlan's pending_empty_ path).
extern "C" int emu_te_msm_many(const uint32_t* bases, uint32_t base_off, size_t m, const uint32_t* scalars, size_t B, int c_in, int T, int T2, int K0,
                               int from_mont, int empty, uint32_t* out) {
  CpuStepBackend be;
  const uint32_t c = c_in ? (uint32_t)c_in : pc::msm_choose_table_c(m, TeFrP::BITS, 0), Wd = pc::msm_num_windows(TeFrP::BITS, c);
  std::vector<uint32_t> table((size_t)Wd * m * Aff::WORDS + 1);
  emu_te_window_table(bases + (size_t)base_off * Aff::WORDS, m, c, Wd, 16, table.data());
  pc::MsmConfig cfg; cfg.T = T;
  if (T2) { cfg.T2 = T2; cfg.T2b = T2 == 4 ? 6 : T2; }
  if (K0) { cfg.K0 = K0; cfg.tbl_K0 = K0; cfg.K1 = K0 == 2 ? 4 : K0; cfg.coop_max_points = 64; cfg.seg_tail_lanes = (T2 == 5) ? 1 : 3; }
  cfg.coop2_max_points = 0;
  cfg.tbl = table.data(); cfg.tbl_c = c; cfg.tbl_stride = (uint32_t)m; cfg.tbl_pt_stride = Aff::WORDS; cfg.tbl_min_n = 0; cfg.tbl_glv = false;
  try {
    pc::MsmPlan<TeC, CpuStepBackend> plan(be, B * m, cfg, (uint32_t)B);
    plan.run(bases, 0, scalars, empty ? 0 : B * m, from_mont != 0, out);
  } catch (const pc::MsmCapacityError&) { return 1; }
  return 0;
}

// what MsmPlan answers to a table or to subs > 0 where it must refuse: 1 if it threw.  kind 0: a twisted Edwards single-MSM plan
// handed a table (stays refused); 1: the many-MSM mode without a table
extern "C" int emu_te_plan_refuses(int kind) {
  CpuStepBackend be;
  uint32_t dummy[Aff::WORDS * 4] = {0};
  pc::MsmConfig cfg;
  try {
    if (kind == 0) { cfg.tbl = dummy; cfg.tbl_c = 8; cfg.tbl_stride = 1; cfg.tbl_pt_stride = Aff::WORDS; pc::MsmPlan<TeC, CpuStepBackend> plan(be, 4, cfg); }
    else { pc::MsmPlan<TeC, CpuStepBackend> plan(be, 4, cfg, 2); }
  } catch (const std::runtime_error&) { return 1; }
  return 0;
}
