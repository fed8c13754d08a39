// TEST-ONLY host compilation of the streaming_kzg kernels (csrc/skzg.hpp): the folding tree (FoldPairBody per level above the tile,
// FoldTailTile below it) and the division by a vanishing polynomial (DivShortTile up to one tile, the division scan above it), run
// through the product's own orchestration with every lane and every phase stepped on the host: validated against
// tests/harness/skzg.py on a machine without a GPU.  NOT part of the product library.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/skzg.hpp"

struct CpuStepBackend {
  std::vector<uint8_t> ws;
  void* workspace(size_t bytes) { if (ws.size() < bytes) ws.assign(bytes, 0); return ws.data(); }
  void sync() {}
  void copy_d2d(void* d, const void* s, size_t bytes) { memcpy(d, s, bytes); }
  void copy_d2h(void* d, const void* s, size_t bytes) { memcpy(d, s, bytes); }
  void copy_h2d(void* d, const void* s, size_t bytes) { memcpy(d, s, bytes); }
  template <class B> void launch(const B& body, size_t lanes) { for (size_t i = 0; i < lanes; i++) body((uint32_t)i); }
};
struct Level { const uint32_t* src; uint32_t len; uint32_t* q; };

extern "C" uint32_t emu_skzg_tile() { return pc::SKZG_TILE_ELEMS; }

template <class FrP>
static uint32_t fold(const uint32_t* f, size_t n, const uint32_t* rho, uint32_t depth, uint32_t* out, const uint64_t* offs) {
  CpuStepBackend be;
  return pc::fold_tree<FrP>(be, f, n, rho, depth, out, offs);
}
// every level of the tree into out at the element offsets offs; returns the number of launches
extern "C" uint32_t emu_skzg_fold_tree(int curve, const uint32_t* f, size_t n, const uint32_t* rho, uint32_t depth, uint32_t* out, const uint64_t* offs) {
  return curve == 0 ? fold<pc_bls12_381_fr>(f, n, rho, depth, out, offs) : fold<pc_bn254_fr>(f, n, rho, depth, out, offs);
}

template <class FrP>
static uint32_t divide(const uint32_t* const* polys, const uint32_t* lens, size_t count, const uint32_t* z, uint32_t k, uint32_t* const* quots, uint32_t* rems) {
  CpuStepBackend be;
  size_t max_len = 0;
  std::vector<Level> lv(count);
  std::vector<std::vector<uint32_t>> q(count);
  for (size_t i = 0; i < count; i++) {
    max_len = std::max<size_t>(max_len, lens[i]);
    q[i].assign((size_t)(1 + (lens[i] > k ? lens[i] - k : 0)) * FrP::N, 0xA5A5A5A5u);      // the slot in front and the quotient
    lv[i] = Level{polys[i], lens[i], q[i].data() + FrP::N};
  }
  std::vector<uint8_t> scratch((2 * max_len + count * k + k) * 32 + count * 24 + 64);
  const uint32_t launches = pc::div_multi<FrP>(be, lv.data(), count, z, k, rems, scratch.data(), 16u);
  for (size_t i = 0; i < count; i++) memcpy(quots[i], q[i].data() + FrP::N, q[i].size() * 4 - (size_t)FrP::N * 4);
  return launches;
}
// `count` polynomials divided by prod (x - z_j): quotients (max(len - k, 0) coefficients each) and remainders (count x k, highest first)
extern "C" uint32_t emu_skzg_div_multi(int curve, const uint32_t* const* polys, const uint32_t* lens, size_t count, const uint32_t* z, uint32_t k,
                                       uint32_t* const* quots, uint32_t* rems) {
  return curve == 0 ? divide<pc_bls12_381_fr>(polys, lens, count, z, k, quots, rems) : divide<pc_bn254_fr>(polys, lens, count, z, k, quots, rems);
}
