// The host side of the two group-generic launches MultilinearPC's setup and the KZG SRS generation share: the fixed-base batch
// multiplication and the pair sums.  G is a curve or G2Of<curve>; the units that instantiate a group's kernels (curve_<name>.hip
// for G1, abi_g2.hip for G2) call them with that group.
#pragma once
#include <algorithm>
#include <vector>
#include "hip_backend.hpp"
#include "msm.hpp"
#include "g2.hpp"
#include "ipa.hpp"

namespace pc {

// out[b] = in[2b] + in[2b + 1], b < count, for affine points of G on the device (PairSumsBody).  Slabs of 2^19 pairs: 252 MB of
// workspace for G2 (an XYZZ sum and a prefix product per pair) whatever the key's size.  A lane adds and normalises K pairs around
// ONE inversion, and the inversion is most of a lane's run time: K = 8 only where that still leaves 2^16 lanes (one wave on every
// SIMD; these kernels hold one wave per SIMD for G2), fewer pairs per lane below -- with K = 8 and slabs of 2^17 throughout, every
// launch was a quarter-filled machine waiting for 16384 serial chains (the upper levels of pc_hip_ml_setup took as long as the 2^nv
// G2 multiplications of level 0).  `in` and `out` must not overlap.
template <class G>
void pair_sums_run(HipBackend& be, const uint32_t* in, size_t count, uint32_t* out) {
  constexpr int AW = AffD<G>::WORDS, XW = XyzzD<G>::WORDS;
  const size_t SLAB = (size_t)1 << 19;
  for (size_t first = 0; first < count; first += SLAB) {
    const size_t cnt = std::min(SLAB, count - first);
    const uint32_t K = (uint32_t)std::min<size_t>(8, std::max<size_t>(1, cnt >> 16));
    uint32_t* ws = (uint32_t*)be.workspace(cnt * (size_t)(XW + AW / 2) * 4);
    PairSumsBody<G> b{in + 2 * first * (size_t)AW, ws, ws + cnt * (size_t)XW, out + first * (size_t)AW, (uint32_t)cnt, K};
    be.launch(b, (cnt + K - 1) / K, 64);
  }
}

// out[i] = scalars[i] * base, i < n: `base.batch_mul(scalars)` for one affine point of G (host) and n Montgomery scalars on the
// device; affine results on the device.  In slabs: an XYZZ result over Fq2 is 384 bytes, so the results of one slab (2^18: 126 MB
// with the prefix products for G2) are normalised before the next slab's are made and the workspace does not grow with n.  Below
// FIXED_BASE_LADDER_BELOW scalars the table (4096 group additions on the host) costs more than it saves: each lane runs its own
// double-and-add ladder.  The table path's normalisation inverts once per K results, so a slab's normalisation is 2^18 / K lanes of
// serial inversion chains: K is the caller's (FIXED_BASE_K_KZG, FIXED_BASE_K_ML in pc_internal.hpp; profiles/EXPERIMENTS.md 000000
// has the measurements of both at 2^20).
constexpr size_t FIXED_BASE_LADDER_BELOW = 4096, FIXED_BASE_SLAB = (size_t)1 << 18;
template <class G>
void fixed_base_run(HipBackend& be, const uint32_t* base, const uint32_t* scalars, size_t n, uint32_t* out, uint32_t K) {
  constexpr int AW = AffD<G>::WORDS, XW = XyzzD<G>::WORDS, FW = AW / 2, FR_W = G::FrP::N;
  if (!n) return;
  if (n < FIXED_BASE_LADDER_BELOW) {
    uint32_t* ws = (uint32_t*)be.workspace(((size_t)AW + n * (size_t)(XW + FW)) * 4);
    uint32_t* dres = ws + AW;
    be.copy_h2d(ws, base, (size_t)AW * 4);
    ScalarMulStoreBody<G> body{{ws, scalars, 1u}, dres};
    be.launch(body, n, 64);
    XyzzBatchAffineBody<G> nb{dres, dres + n * (size_t)XW, out, (uint32_t)n, 1};
    be.launch(nb, n, 64);
    be.sync();
    return;
  }
  // window table of the fixed base on the host: T[w][d-1] = d * 2^(8 w) * base, d = 1..128 (one inversion for all of it)
  const uint32_t Wd = msm_num_windows(G::FrP::BITS, FIXED_BASE_C);
  std::vector<uint32_t> tbl;
  host64::fixed_base_window_table<G>(base, FIXED_BASE_C, Wd, tbl);
  // device: table | XYZZ results of one slab | their prefix products
  const size_t slab = std::min(n, FIXED_BASE_SLAB), tb = tbl.size() * 4;
  uint8_t* ws = (uint8_t*)be.workspace(tb + slab * (size_t)(XW + FW) * 4);
  uint32_t* dtbl = (uint32_t*)ws; uint32_t* dres = (uint32_t*)(ws + tb); uint32_t* dscr = dres + slab * (size_t)XW;
  be.copy_h2d(dtbl, tbl.data(), tb);
  for (size_t first = 0; first < n; first += slab) {
    const size_t cnt = std::min(slab, n - first);
    FixedBaseTableMulBody<G> body{scalars + first * (size_t)FR_W, dtbl, Wd, dres};
    be.launch(body, cnt, 64);
    XyzzBatchAffineBody<G> nb{dres, dscr, out + first * (size_t)AW, (uint32_t)cnt, K};
    be.launch(nb, (cnt + K - 1) / K, 64);
  }
  be.sync();                                   // the host table goes out of scope
}

}  // namespace pc
