// G2 of a pairing curve on the device: the kernel bodies beside the MSM that MultilinearPC (XZZPD19,
// poly-commit/src/multilinear_pc/mod.rs) needs.
//
// The G2 MSM itself is MsmPlan<G2Of<C>, Backend> (msm.hpp): the same "sort, then segment" pipeline as G1 -- the digit and sort stages
// are the pairing curve's own (they only look at scalars), accumulate / segmented reduction / bucket reduction are instantiated for
// XYZZ points over Fq2 (fp2.hpp; 96 words a bucket, 48 an affine base) and the host tail folds the <= 40 partial sums over
// host64::F64x2.  It replaces <E::G2 as VariableBaseMSM>::msm_bigint (multilinear_pc/mod.rs:162-163).
// TABLE-FREE ONLY: no window table, no GLV (psi) split, no radix-2^30 running sum, no captured launch graphs and no host-parts
// split exist for G2; every coordinate is canonical (no lazy [0, 2p) forms).
#pragma once
#include "ec.hpp"

namespace pc {

// out[b] = in[2b] + in[2b + 1] as affine points, b < count: the pair sums of a MultilinearPC key (every q[b] of an opening
// multiplies H[2b] + H[2b + 1], mod.rs:158-160).  One inversion per lane for its K pairs (JacBatchAffineBody's scheme, ec.hpp: the
// prefix products of ZZ * ZZZ are parked in `scratch`, inverted once, peeled off backwards).  All special cases are the group
// law's: P + P doubles, P + (-P) and infinity + infinity give the all-zero point, infinity + P gives P.
template <class G>
struct PairSumsBody {
  typedef XyzzD<G> Pt;
  typedef typename Pt::Fq Fq;
  static constexpr int AW = AffD<G>::WORDS, FN = Fq::N;
  const uint32_t* in;       // 2 * count affine points
  uint32_t* sums;           // count XYZZ points (scratch)
  uint32_t* scratch;        // count coordinates (scratch)
  uint32_t* out;            // count affine points
  uint32_t count, K;
  PC_HD void operator()(uint32_t t) const {
    const uint32_t s = t * K, e = (count - s > K) ? s + K : count;
    Fq run = Fq::one();
    for (uint32_t j = s; j < e; j++) {
      Pt p = Pt::from_affine(AffD<G>::load(in + (size_t)(2 * j) * AW));
      p.add_affine(AffD<G>::load(in + (size_t)(2 * j + 1) * AW));
      p.store(sums + (size_t)j * Pt::WORDS);
      run.store(scratch + (size_t)j * FN);
      if (!p.is_inf()) run = run.mul(p.ZZ.mul(p.ZZZ));
    }
    Fq inv = run.inv();
    for (uint32_t j = e; j-- > s;) {
      const Pt p = Pt::load(sums + (size_t)j * Pt::WORDS);
      AffD<G> a = AffD<G>::infinity();
      if (!p.is_inf()) {
        const Fq ti = inv.mul(Fq::load(scratch + (size_t)j * FN));      // 1 / (ZZ * ZZZ) of pair j
        inv = inv.mul(p.ZZ.mul(p.ZZZ));
        a.x = p.X.mul(ti.mul(p.ZZZ)); a.y = p.Y.mul(ti.mul(p.ZZ));
      }
      a.store(out + (size_t)j * AW);
    }
  }
};

// One halving round of MultilinearPC::open (mod.rs:153-157), Montgomery in and out:
//   q[b] = r[2b + 1] - r[2b],   r_out[b] = r[2b] (1 - z) + r[2b + 1] z = r[2b] + z q[b]     (field elements: the same values)
// r_out must not alias r_in: lane b writes what lane b / 2 reads.
template <class FrP>
struct MlFoldBody {
  typedef Fd<FrP> Fr;
  const uint32_t* r_in; uint32_t* r_out; uint32_t* q;
  uint32_t z[FrP::N];
  PC_HD void operator()(uint32_t b) const {
    const Fr lo = Fr::load(r_in + (size_t)(2 * b) * FrP::N), hi = Fr::load(r_in + (size_t)(2 * b + 1) * FrP::N);
    const Fr d = hi.sub(lo);
    d.store(q + (size_t)b * FrP::N);
    lo.add(Fr::load(z).mul(d)).store(r_out + (size_t)b * FrP::N);
  }
};

// The eq table of MultilinearPC::setup (eq_extension and the running products of mod.rs:36-51, 219-234), Montgomery in and out:
//   out[x] = prod_{j < nv} e(t_j, bit_j(x)),   e(t, 0) = 1 - t,  e(t, 1) = t
// one lane per x; both factors of every variable travel in the body (2 x 30 x 8 words).  Level i of the reference's eq_arr is the
// same table over t[i ..]; out[2b] + out[2b + 1] is the table of t[1 ..] at b.
static constexpr uint32_t ML_MAX_VARS = 30;
template <class FrP>
struct MlEqBody {
  typedef Fd<FrP> Fr;
  uint32_t* out;
  uint32_t nv;
  uint32_t e[ML_MAX_VARS][2][FrP::N];      // e[j][b] = e(t_j, b)
  void set_point(const uint32_t* t_mont, uint32_t n_vars) {
    nv = n_vars;
    for (uint32_t j = 0; j < n_vars; j++) {
      const Fr tj = Fr::load(t_mont + (size_t)j * FrP::N);
      Fr::one().sub(tj).store(e[j][0]); tj.store(e[j][1]);
    }
  }
  PC_HD void operator()(uint32_t x) const {
    // (both factors are loaded with wave-uniform addresses and selected per lane)
    Fr acc = fq_sel((x & 1) != 0, Fr::load(e[0][1]), Fr::load(e[0][0]));
    for (uint32_t j = 1; j < nv; j++) acc = acc.mul(fq_sel(((x >> j) & 1) != 0, Fr::load(e[j][1]), Fr::load(e[j][0])));
    acc.store(out + (size_t)x * FrP::N);
  }
};

// k * P for one lane: the late rounds of an opening (a handful of pairs) are launch-latency bound in the full pipeline, so each lane
// multiplies its own pair by double-and-add from the top bit (XYZZ) and a workgroup tree adds the products (abi_g2.hip).
template <class G>
struct ScalarMulBody {
  typedef XyzzD<G> Pt;
  typedef typename G::FrP FrP;
  static constexpr int AW = AffD<G>::WORDS;
  const uint32_t* bases; const uint32_t* scalars;      // n affine points, n Montgomery scalars
  uint32_t from_mont;
  PC_HD Pt product(uint32_t j) const {
    Fd<FrP> k = Fd<FrP>::load(scalars + (size_t)j * FrP::N);
    if (from_mont) k = k.from_mont();
    const AffD<G> p = AffD<G>::load(bases + (size_t)j * AW);
    Pt acc = Pt::infinity();
    // (the scalar is shifted through its top bit with compile-time limb indices: a run-time index would put it into scratch memory)
    for (int bit = 0; bit < 32 * FrP::N; bit++) {
      const uint32_t top = k.l[FrP::N - 1] >> 31;
      PC_UNROLL for (int i = FrP::N - 1; i > 0; i--) k.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);
      k.l[0] <<= 1;
      acc = acc.dbl();
      if (top) acc.add_affine(p);
    }
    return acc;
  }
};

// The same ladder with the product stored: a fixed-base multiplication of a handful of scalars (no window table to build), one base
// for every lane; normalised by XyzzBatchAffineBody.
template <class G>
struct ScalarMulStoreBody {
  ScalarMulBody<G> m;        // bases: ONE affine point
  uint32_t* out_xyzz;
  PC_HD void operator()(uint32_t j) const {
    ScalarMulBody<G> one = m;
    one.scalars = m.scalars + (size_t)j * G::FrP::N;
    one.product(0).store(out_xyzz + (size_t)j * XyzzD<G>::WORDS);
  }
};
}  // namespace pc
