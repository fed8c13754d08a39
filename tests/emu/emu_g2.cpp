// TEST-ONLY host compilation of the G2 headers (fp2.hpp, the XYZZ law over Fq2, g2.hpp) and of the MSM orchestration of msm.hpp
// instantiated for G2Of<BLS12-381>, stepped lane by lane by a single-threaded backend: the indexing logic and the arithmetic are
// validated against tests/harness/g2ref.py on a machine without a GPU.  NOT part of the product library.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/msm.hpp"
#include "../../poly_commit_amd/csrc/g2.hpp"

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

typedef pc::G2Of<pc_curve_bls12_381> G2C;
typedef pc::Fq2D<pc_bls12_381_fq> Fq2;
typedef pc::XyzzD<G2C> Pt;
typedef pc::AffD<G2C> Aff;

// Fq2 operations on 24-word elements: 0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 inv, 6 mul_add_mul (a b + c d), 7 dbl
extern "C" void emu_g2_fop(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
  const Fq2 A = Fq2::load(a), B = Fq2::load(b);
  Fq2 r;
  switch (op) {
    case 0: r = A.mul(B); break;
    case 1: r = A.sqr(); break;
    case 2: r = A.add(B); break;
    case 3: r = A.sub(B); break;
    case 4: r = A.neg(); break;
    case 5: r = A.inv(); break;
    case 6: r = A.mul_add_mul(B, Fq2::load(c), Fq2::load(d)); break;
    default: r = A.dbl(); break;
  }
  r.store(out);
}

// group law on affine inputs (48 words each), affine output.  zz != 0: both operands are first brought to a representative with a
// non-trivial ZZ, (P + X) + (-X) through the mixed and the full addition (X = aux, any point).
//   op 0: P + Q mixed (add_affine)   1: P + Q full (add)   2: 2 P (dbl)   3: 2 P from affine (dbl_affine)
extern "C" void emu_g2_ecop(int op, int zz, const uint32_t* a, const uint32_t* b, const uint32_t* aux, uint32_t* out) {
  const Aff A = Aff::load(a), B = Aff::load(b), X = Aff::load(aux);
  Pt p = Pt::from_affine(A), q = Pt::from_affine(B);
  if (zz) {
    p.add_affine(X); p.add(Pt::from_affine(X.neg_if(true)));
    q.add_affine(X); q.add(Pt::from_affine(X.neg_if(true)));
  }
  Pt r;
  switch (op) {
    case 0: r = p; r.add_affine(B); break;
    case 1: r = p; r.add(q); break;
    case 2: r = p.dbl(); break;
    default: r = Pt::dbl_affine(A); break;
  }
  r.to_affine().store(out);
}

extern "C" int emu_g2_msm(const uint32_t* bases, size_t n_srs, const uint32_t* scalars, size_t n, uint32_t base_off, int c, int T, int T2, int K0,
                          int from_mont, uint32_t* out) {
  CpuStepBackend be;
  pc::MsmConfig cfg; cfg.c = c; cfg.T = T;
  if (T2) { cfg.T2 = T2; cfg.T2b = T2 == 4 ? 6 : T2; }
  if (K0) { cfg.K0 = K0; cfg.K1 = K0 == 2 ? 4 : K0; cfg.coop_max_points = 64; cfg.seg_tail_lanes = (T2 == 5) ? 1 : 3; }
  cfg.coop2_max_points = 0;
  try {
    pc::MsmPlan<G2C, CpuStepBackend> plan(be, n_srs, cfg);
    plan.run(bases, base_off, scalars, n, from_mont != 0, out);
  } catch (const pc::MsmCapacityError&) { return 1; }
  return 0;
}

extern "C" void emu_g2_pair_sums(const uint32_t* in, size_t count, uint32_t K, uint32_t* out) {
  std::vector<uint32_t> sums(count * Pt::WORDS + 1), scratch(count * Fq2::N + 1);
  pc::PairSumsBody<G2C> b{in, sums.data(), scratch.data(), out, (uint32_t)count, K};
  CpuStepBackend be; be.launch(b, (count + K - 1) / K);
}

extern "C" void emu_ml_fold(const uint32_t* r_in, size_t n_half, const uint32_t* z, uint32_t* r_out, uint32_t* q) {
  pc::MlFoldBody<pc_bls12_381_fr> b; b.r_in = r_in; b.r_out = r_out; b.q = q;
  memcpy(b.z, z, sizeof(b.z));
  CpuStepBackend be; be.launch(b, n_half);
}

// the per-lane products of the small-round kernel (one XYZZ product per lane), summed and normalised on the host
struct ScalarMulStoreBody {
  pc::ScalarMulBody<G2C> m; uint32_t* out;
  void operator()(uint32_t j) const { m.product(j).store(out + (size_t)j * Pt::WORDS); }
};
extern "C" void emu_g2_small_msm(const uint32_t* bases, const uint32_t* scalars, size_t n, int from_mont, uint32_t* out) {
  std::vector<uint32_t> prod(n * Pt::WORDS + 1);
  ScalarMulStoreBody b{{bases, scalars, from_mont ? 1u : 0u}, prod.data()};
  CpuStepBackend be; be.launch(b, n);
  Pt acc = Pt::infinity();
  for (size_t i = 0; i < n; i++) acc.add(Pt::load(prod.data() + i * Pt::WORDS));
  uint32_t w[Pt::WORDS]; acc.store(w);
  pc::host64::Xyzz64<G2C>::load(w).store_affine(out);
}
