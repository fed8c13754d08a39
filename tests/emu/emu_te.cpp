// TEST-ONLY host compilation of the twisted Edwards headers (te.hpp: the extended-coordinate law, the key fold and its normalisation)
// and of the MSM orchestration of msm.hpp instantiated for TeOf<ed_on_bls12_381>, stepped lane by lane by a single-threaded backend:
// the indexing logic and the arithmetic are validated against tests/harness/teref.py on a machine without a GPU.  NOT part of the
// product library.
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

// group law on points given as x || y (16 words each; all zero: the empty entry), output x || y || 2dxy (24 words) as to_affine makes it.
// ext != 0: both operands are first brought to a representative with Z != 1, (P + X) + (-X) through the mixed and the full addition.
//   op 0: P + Q mixed (add_affine)   1: P + Q full (add)   2: 2 P (dbl)
extern "C" void emu_te_ecop(int op, int ext, const uint32_t* a, const uint32_t* b, const uint32_t* aux, uint32_t* out) {
  const Aff A = Aff::load_xy(a), B = Aff::load_xy(b), X = Aff::load_xy(aux);
  Pt p = Pt::from_affine(A), q = Pt::from_affine(B);
  if (ext) {
    p.add_affine(X); p.add(Pt::from_affine(X.neg_if(true)));
    q.add_affine(X); q.add(Pt::from_affine(X.neg_if(true)));
  }
  Pt r;
  switch (op) {
    case 0: r = p; r.add_affine(B); break;
    case 1: r = p; r.add(q); break;
    default: r = p.dbl(); break;
  }
  r.to_affine().store(out);
}

// the resident form of n points from their x || y (TeDeriveBody), and back (TeStripBody)
extern "C" void emu_te_derive(const uint32_t* xy, size_t n, uint32_t* out) {
  pc::TeDeriveBody<TeC> b{xy, out};
  CpuStepBackend be; be.launch(b, n);
}
extern "C" void emu_te_strip(const uint32_t* res, size_t n, uint32_t* out_xy) {
  pc::TeStripBody<TeC> b{res, out_xy};
  CpuStepBackend be; be.launch(b, n);
}

// the whole pipeline; bases in the resident form, out: x || y (16 words)
extern "C" int emu_te_msm(const uint32_t* bases, size_t n_srs, const uint32_t* scalars, size_t n, uint32_t base_off, int c, int T, int T2, int K0,
                          int from_mont, uint32_t* out) {
  CpuStepBackend be;
  pc::MsmConfig cfg; cfg.c = c; cfg.T = T;
  if (T2) { cfg.T2 = T2; cfg.T2b = T2 == 4 ? 6 : T2; }
  if (K0) { cfg.K0 = K0; cfg.K1 = K0 == 2 ? 4 : K0; cfg.coop_max_points = 64; cfg.seg_tail_lanes = (T2 == 5) ? 1 : 3; }
  cfg.coop2_max_points = 0;
  try {
    pc::MsmPlan<TeC, CpuStepBackend> plan(be, n_srs, cfg);
    plan.run(bases, base_off, scalars, n, from_mont != 0, out);
  } catch (const pc::MsmCapacityError&) { return 1; }
  return 0;
}

// AccumulateBody on a given bucket-sorted entry list: offsets[NB + 1] (CSR), entries[offsets[NB]] (base index | sign << 31), chunks of
// T entries.  Outputs as the kernel leaves them: buckets (NB x 32 words, zero-filled before), pkeys (2 per lane), ppts (2 x 32 words
// per lane).  Returns the number of lanes.
extern "C" uint32_t emu_te_accumulate(const uint32_t* bases, const uint32_t* entries, const uint32_t* offsets, uint32_t NB, uint32_t T,
                                      uint32_t* buckets, uint32_t* pkeys, uint32_t* ppts) {
  pc::MsmGeom g;
  memset(&g, 0, sizeof(g));
  g.NB = NB; g.W = 1; g.nb_win = NB; g.T = T; g.T2 = 4; g.T2b = 4; g.pt_stride = Aff::WORDS; g.c = 2; g.Wd = 1;
  const uint32_t M = offsets[NB], lanes = (M + T - 1) / T;
  memset(buckets, 0, (size_t)NB * Pt::WORDS * 4);
  pc::AccumulateBody<TeC> b{g, bases, entries, offsets, buckets, pkeys, ppts};
  CpuStepBackend be; be.launch(b, lanes);
  return lanes;
}

// one key fold in place on a key in the resident form: TeEcFoldBody, then TeBatchAffineBody with K points per inversion
extern "C" void emu_te_fold(uint32_t* key, size_t half, const uint32_t* u_mont, uint32_t K) {
  std::vector<uint32_t> ext(half * Pt::WORDS + 1), scratch(half * Pt::Fq::N + 1);
  pc::TeEcFoldBody<TeC> f;
  f.key = key; f.half = (uint32_t)half; f.ext = ext.data();
  const pc::Fd<pc_ed_on_bls12_381_fr> u = pc::Fd<pc_ed_on_bls12_381_fr>::load(u_mont).from_mont();
  f.naf.from_scalar(u.l);
  CpuStepBackend be; be.launch(f, half);
  pc::TeBatchAffineBody<TeC> nb{ext.data(), scratch.data(), key, (uint32_t)half, K};
  be.launch(nb, (half + K - 1) / K);
}
