// TEST-ONLY probe of the two-lane XYZZ addition (csrc/msm_coop.hpp half_add, csrc/ec.hpp HalfPt / HalfAdd).
// param = number of cases n.  in = per case P | Q (raw XYZZ words).  out = per case: the sum of the lane pair | the sum of a single lane.
//   lanes [0, 2n)   lane pair (2c, 2c + 1) of case c: operands loaded as HalfPt::of(P, odd), one half_add, each lane stores its halves
//   lanes [2n, 3n)  lane 2n + c: XyzzD::add of the same operands on one lane
// Device: the neighbour exchanges of half_add are DPP moves, and the pairs of a wave take whatever branches their cases ask for.
// Host: both lanes of a pair are stepped through the same phases with the exchanges as plain assignments (as tests/emu does).
#pragma once
#include "../../poly_commit_amd/csrc/ec.hpp"
#if defined(__HIPCC__)
#include "../../poly_commit_amd/csrc/hip_backend.hpp"      // (msm_coop.hpp's kernels use its PC_LATENCY_KERNEL)
#include "../../poly_commit_amd/csrc/msm_coop.hpp"
#endif

namespace probe {
using namespace pc;

template <class C>
struct HalfAddBody {
  typedef XyzzD<C> Pt; typedef HalfPt<C> H; typedef Fd<typename C::FqP> Fq;
  static constexpr int FN = Fq::N, IN_WORDS = 8 * FN, OUT_WORDS = 8 * FN;
  const uint32_t* in; uint32_t* out; const uint32_t* aux; uint32_t param;
  PC_HD void single(uint32_t c) const {
    Pt r = Pt::load(in + (size_t)c * IN_WORDS);
    r.add(Pt::load(in + (size_t)c * IN_WORDS + 4 * FN));
    r.store(out + (size_t)c * OUT_WORDS + 4 * FN);
  }
  PC_HD void operator()(uint32_t lane) const {
    const uint32_t n = param;
    if (lane >= 2 * n) { if (lane - 2 * n < n) single(lane - 2 * n); return; }
    const uint32_t c = lane >> 1;
    const Pt P = Pt::load(in + (size_t)c * IN_WORDS), Q = Pt::load(in + (size_t)c * IN_WORDS + 4 * FN);
    uint32_t* o = out + (size_t)c * OUT_WORDS;
#if defined(__HIP_DEVICE_COMPILE__)
    const bool odd = (lane & 1u) != 0;
    H p = H::of(P, odd);
    half_add<C>(p, H::of(Q, odd), odd);
    p.a.store(o + (odd ? FN : 0)); p.b.store(o + (odd ? 3 * FN : 2 * FN));
#else
    if (lane & 1u) return;                       // the even lane steps the pair
    H p[2] = {H::of(P, false), H::of(P, true)};
    const H q[2] = {H::of(Q, false), H::of(Q, true)};
    if (q[0].b.is_zero()) { /* + infinity */ }
    else if (p[0].b.is_zero()) { p[0] = q[0]; p[1] = q[1]; }
    else {
      HalfAdd<C> h[2];
      const bool pz = h[0].p1(p[0], q[0]), rz = h[1].p1(p[1], q[1]);      // even lane: P == 0, odd lane: R == 0
      if (pz) {
        Pt f; f.X = p[0].a; f.ZZ = p[0].b; f.Y = p[1].a; f.ZZZ = p[1].b;
        const Pt r = rz ? f.dbl() : Pt::infinity();
        p[0] = H::of(r, false); p[1] = H::of(r, true);
      } else {
        const Fq s0 = h[0].p2(p[0], q[0], false), s1 = h[1].p2(p[1], q[1], true);
        const Fq t0 = h[0].p3(false, s1), t1 = h[1].p3(true, s0);
        h[0].p4(p[0], false, t1); h[1].p4(p[1], true, t0);
      }
    }
    p[0].a.store(o); p[1].a.store(o + FN); p[0].b.store(o + 2 * FN); p[1].b.store(o + 3 * FN);
#endif
  }
};

}  // namespace probe
