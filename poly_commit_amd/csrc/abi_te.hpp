// What the three units of the twisted Edwards ABI share (abi_te.hip, abi_te_ipa.hip, abi_te_setup.hip): the names and sizes of
// ed_on_bls12_381, the id check, and the normalisation that ends every launch sequence which makes key points.  Nothing here
// instantiates a kernel by being included.
#pragma once
#include "abi.hpp"
#include "te.hpp"

namespace pc {

typedef TeOf<pc_te_ed_on_bls12_381> TeC;
typedef TeC::FrP TeFrP;
constexpr int TE_AW = AffD<TeC>::WORDS, TE_XY = AffD<TeC>::XY_WORDS, TE_XW = XyzzD<TeC>::WORDS, TE_FR_W = TeFrP::N, TE_FQ_W = TeC::FqP::N;
constexpr size_t TE_POINT_BYTES = (size_t)TE_XY * 4;      // the caller's x || y
constexpr size_t TE_FR_BYTES = (size_t)TE_FR_W * 4;
constexpr uint32_t TE_NORM_K = 16;                        // points per inversion of a normalisation (JacBatchAffineBody's default)

// The backend's workspace for a launch sequence that ends in te_normalise over n points: n extended points | the n prefix products
// of the normalisation | `extra_words` words of the caller's
struct TeNormBuf { uint32_t* ext; uint32_t* scratch; uint32_t* extra; };
inline TeNormBuf te_norm_buf(HipBackend& be, size_t n, size_t extra_words = 0) {
  uint32_t* ext = (uint32_t*)be.workspace((n * (size_t)(TE_XW + TE_FQ_W) + extra_words) * 4);
  return TeNormBuf{ext, ext + n * (size_t)TE_XW, ext + n * (size_t)(TE_XW + TE_FQ_W)};
}
// n extended points -> the resident form at dst (TeBatchAffineBody), queued behind whatever wrote ext; the caller drains the queue.
// (A template so that a unit which never normalises instantiates no kernel.)
template <class Backend>
void te_normalise(Backend& be, const uint32_t* ext, uint32_t* scratch, uint32_t* dst, size_t n) {
  TeBatchAffineBody<TeC> nb{ext, scratch, dst, (uint32_t)n, TE_NORM_K};
  be.launch(nb, (n + TE_NORM_K - 1) / TE_NORM_K);
}

}  // namespace pc

inline int te_curve_check(pc_te_curve curve) { return curve == PC_TE_ED_ON_BLS12_381 ? PC_OK : PC_ERR_INVALID_ARG; }
