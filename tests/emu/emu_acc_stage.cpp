// TEST-ONLY: AccumulateBody<pc_curve_bls12_381>::chunk (poly_commit_amd/csrc/msm.hpp) stepped lane by lane on the host with the
// two staging policies of the prefetched base: StageRegs (what every host caller and every kernel but the radix-2^30 one uses) and a
// host stand-in of the device's StageLds (msm_coop.hpp): an array indexed like the workgroup's exchange tile (acc_stage_word), one
// slot per workgroup lane, written by gather() and read back by take().  Not part of the product library.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../poly_commit_amd/csrc/msm.hpp"

namespace {
typedef pc_curve_bls12_381 C;
typedef pc::AccumulateBody<C> Body;
constexpr uint32_t WG = 256, AW = pc::AffD<C>::WORDS, PIECES = AW / 4;

struct StageTileHost {
  uint32_t* tile; uint32_t tid;          // tile: PIECES * 4 * WG words, shared by the lanes of one workgroup
  void gather(const uint32_t* src) const {
    for (uint32_t j = 0; j < PIECES; j++) memcpy(tile + pc::acc_stage_word(tid, j, PIECES), src + 4 * j, 16);
  }
  pc::AffD<C> take() const {
    uint32_t w[AW];
    for (uint32_t j = 0; j < PIECES; j++) memcpy(w + 4 * j, tile + pc::acc_stage_word(tid, j, PIECES), 16);
    return pc::AffD<C>::load(w);
  }
  void done() const {}
};
}  // namespace

// policy 0: registers, 1: the tile.  Outputs: buckets (NB points), pkeys (2 per lane), ppts (2 points per lane), last (1 point per
// lane: the register copy of the lane's last run), all as the kernel leaves them.  Returns the number of tile words that two lanes
// of one workgroup both wrote (must be 0: the slots are disjoint).
extern "C" int emu_acc_stage_chunks(const uint32_t* bases, uint32_t pt_stride, const uint32_t* entries, const uint32_t* offsets, uint32_t NB,
                                    uint32_t T, uint32_t lanes, int policy, uint32_t* buckets, uint32_t* pkeys, uint32_t* ppts, uint32_t* last) {
  pc::MsmGeom g; memset(&g, 0, sizeof g);
  g.NB = NB; g.T = T; g.pt_stride = pt_stride; g.W = 1; g.nb_win = NB;
  Body b{g, bases, entries, offsets, buckets, pkeys, ppts};
  constexpr uint32_t PW = Body::Pt::WORDS;
  std::vector<uint32_t> tile(AW * WG), owner(AW * WG);
  int shared_words = 0;
  for (uint32_t t = 0; t < lanes; t++) {
    const uint32_t tid = t % WG;
    if (tid == 0) { std::fill(tile.begin(), tile.end(), 0xdeadbeefu); std::fill(owner.begin(), owner.end(), 0xffffffffu); }
    uint32_t k0, k1; Body::Pt v = Body::Pt::infinity();
    if (policy == 0) b.chunk(t, k0, k1, v);
    else {
      for (uint32_t j = 0; j < PIECES; j++)
        for (uint32_t q = 0; q < 4; q++) {
          uint32_t& o = owner[pc::acc_stage_word(tid, j, PIECES) + q];
          if (o != 0xffffffffu && o != tid) shared_words++;
          o = tid;
        }
      b.chunk(t, k0, k1, v, StageTileHost{tile.data(), tid});
    }
    pkeys[2 * t] = k0; pkeys[2 * t + 1] = k1;
    v.store(last + (size_t)t * PW);
  }
  return shared_words;
}

// one bucket (XYZZ, possibly lazily reduced) as a canonical affine point
extern "C" void emu_acc_stage_affine(const uint32_t* xyzz, uint32_t* out) { Body::Pt::load(xyzz).canonical().to_affine().store(out); }
// the tile word where piece j of workgroup lane tid's slot begins
extern "C" uint32_t emu_acc_stage_word(uint32_t tid, uint32_t j) { return pc::acc_stage_word(tid, j, PIECES); }
