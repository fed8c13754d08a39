// The blocking MSM lane of a group that has no asynchronous pipeline (G2, twisted Edwards): BlockingRunner over MsmPlan<G, HipBackend>.
// Only the unit that instantiates everything of its group includes this (abi_g2.hip for G2Of<C>, abi_te.hip for TeOf<T>): the plan and
// its kernels are instantiated there and nowhere else.
#pragma once
#include "hip_backend_msm.hpp"
#include "key.hpp"

namespace pc {

// Plain launches (no captured graphs), host scalars staged whole (no parts).  subs == 0: one MSM per run; subs == B: the many-MSM pass
// against cfg's window table (`run` then takes B x m scalars and writes B points)
template <class G>
struct BlockingRunnerT : BlockingRunner {
  HipBackend& be;
  MsmPlan<G, HipBackend> plan;
  BlockingRunnerT(HipBackend& b, size_t n_max, const MsmConfig& cfg, uint32_t subs) : be(b), plan(b, n_max, cfg, subs) {}
  void run(const uint32_t* bases, uint32_t base_off, const void* scalars, pc_mem where, size_t n, bool from_mont, uint32_t* out_host) override {
    const uint32_t* sdev = (const uint32_t*)scalars;
    be.n_ev = 0; be.mark();
    if (where == PC_MEM_HOST && n) { be.copy_h2d(plan.scalar_staging(), scalars, n * (size_t)G::FrP::N * 4); sdev = plan.scalar_staging(); }
    plan.run(bases, base_off, sdev, n, from_mont, out_host);
  }
  void shape(uint32_t out[4]) const override {
    const MsmGeom& g = plan.last_geom();
    out[0] = g.c; out[1] = g.Wd; out[2] = g.NB; out[3] = g.tbl_stride ? 1u : 0u;
  }
};

// A new lane for up to n_max pairs.  cfg is the caller's: the context's with the group's own settings and either no table or the
// table of the many-MSM pass (subs bucket sets)
template <class G>
BlockingLane* blocking_lane(size_t n_max, MsmConfig cfg, uint32_t subs) {
  BlockingLane* L = new BlockingLane();
  try {
    L->be.init();
    cfg.coop2_max_points = 0;      // one lane per point in every cooperative level (the two-lane form is a G1 schedule)
    L->runner = new BlockingRunnerT<G>(L->be, n_max, cfg, subs);
  } catch (...) { delete L; throw; }
  return L;
}

}  // namespace pc
