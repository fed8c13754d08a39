// Scalar-field kernels of streaming_kzg: the folding tree of Gemini's tensor check and the division by a vanishing polynomial
// with its remainder.
//
// folding tree (FoldedPolynomialTree, poly-commit/src/streaming_kzg/data_structures.rs:12-138), in natural order (index = degree):
//   f_0 = f,  L_i = ceil(n / 2^i),  f_i[b] = f_{i-1}[2b] + rho_{i-1} * f_{i-1}[2b + 1]   (a coefficient past the end is zero)
// division (CommitterKeyStream::open_multi_points, streaming_kzg/space.rs:98-136): q = p div Z, r = p mod Z, Z = prod_j (x - z_j).
//   q is k successive synthetic divisions by (x - z_j); the remainders c_j of those divisions are the NEWTON coefficients of r:
//   r = c_0 + c_1 (x - z_0) + c_2 (x - z_0)(x - z_1) + ...   (the host turns them into monomial coefficients, k^2 products)
//
// Launch structure.  A level of the tree longer than one tile is one launch (FoldPairBody: lane b reads the pair 2b, 2b + 1 -- 64
// contiguous bytes -- and writes element b).  From the first level of at most SKZG_TILE coefficients on, ONE launch of one workgroup
// makes every remaining level (FoldTailTile): the tile stays in LDS and every level is written out.  The division of a polynomial of
// at most one tile is one workgroup as well (DivShortTile; pc_hip_kzg_open_folding divides ALL its short levels in one launch, one
// workgroup per level): the division scan of poly.hpp with the fan-ins 4 x 16 x 16 inside LDS, k passes in place.  Longer
// polynomials take k runs of div_scan.
//
// SKZG_TILE = 1024 coefficients (32 KiB): FoldTailTile keeps 1.5 tiles (48 KiB), DivShortTile one tile and 2 x 256 + 2 x 16 partial
// values (49 KiB) of the 160 KiB of LDS of a CU; 256 lanes = four wave64, CH = 4 coefficients per lane.
//
// Both tiles are written as PHASES (phase p of lane tid; a workgroup barrier between phases) so that tests/emu steps exactly the
// code the kernels run.
#pragma once
#include <algorithm>
#include <vector>
#include "fp32.hpp"
#include "poly.hpp"

namespace pc {

static constexpr uint32_t SKZG_TILE_ELEMS = 1024, SKZG_LANES = 256, SKZG_CH = SKZG_TILE_ELEMS / SKZG_LANES, SKZG_GRP = 16;
static_assert(SKZG_LANES == SKZG_GRP * SKZG_GRP && SKZG_CH * SKZG_LANES == SKZG_TILE_ELEMS, "the tile is 16 groups of 16 lanes of CH coefficients");

// one level above the tile: out[b] = src[2b] + rho * src[2b + 1], b < ceil(len / 2)
template <class FrP>
struct FoldPairBody {
  typedef Fd<FrP> F;
  const uint32_t* src; uint32_t len; F rho; uint32_t* out;
  PC_HD void operator()(uint32_t b) const {
    const size_t i = (size_t)2 * b;
    F a = F::load(src + i * FrP::N);
    if (i + 1 < len) a = a.add(rho.mul(F::load(src + (i + 1) * FrP::N)));
    a.store(out + (size_t)b * FrP::N);
  }
};

// ceil(len / 2^j) for len >= 1
PC_HD uint32_t skzg_level_len(uint32_t len, uint32_t j) { return j >= 32 ? 1u : (uint32_t)((((uint64_t)len - 1) >> j) + 1); }

// every level below a source level of at most one tile: phase 0 loads the source into A, phase j (1 .. levels) makes level j from
// level j - 1 (A -> B -> A ...: level j has at most TILE / 2^j coefficients, B holds TILE / 2) and writes it to out + offs[j - 1]
template <class FrP>
struct FoldTailTile {
  typedef Fd<FrP> F;
  const uint32_t* src; uint32_t len;      // 1 <= len <= SKZG_TILE_ELEMS
  const uint32_t* rho;                    // `levels` challenges (device)
  const uint64_t* offs;                   // `levels` element offsets into out (device)
  uint32_t levels; uint32_t* out;
  PC_HD uint32_t phases() const { return levels + 1; }
  PC_HD void phase(uint32_t p, uint32_t* A, uint32_t* B, uint32_t tid, uint32_t nthr) const {
    if (p == 0) {
      for (uint32_t i = tid; i < len; i += nthr) F::load(src + (size_t)i * FrP::N).store(A + (size_t)i * FrP::N);
      return;
    }
    const uint32_t* cur = (p & 1) ? A : B; uint32_t* nxt = (p & 1) ? B : A;
    const uint32_t cur_len = skzg_level_len(len, p - 1), out_len = skzg_level_len(len, p);
    const F r = F::load(rho + (size_t)(p - 1) * FrP::N);
    uint32_t* o = out + (size_t)offs[p - 1] * FrP::N;
    for (uint32_t b = tid; b < out_len; b += nthr) {
      F a = F::load(cur + (size_t)2 * b * FrP::N);
      if (2 * b + 1 < cur_len) a = a.add(r.mul(F::load(cur + ((size_t)2 * b + 1) * FrP::N)));
      a.store(nxt + (size_t)b * FrP::N); a.store(o + (size_t)b * FrP::N);
    }
  }
};

// One polynomial of at most one tile divided by Z in LDS.  Pass j divides X[j .. len) by (x - z_j) in place: afterwards X[j] is the
// Newton coefficient c_j and X[j + 1 .. len) the quotient so far.  A pass is the division scan in five phases: lane t owns the
// coefficients [CH t, CH t + CH); U: its Horner value with carry-in 0; G: lanes < 16 fold 16 of those with z^CH; C: lane 0 chains the
// 16 group values with z^(16 CH) into the carries of the groups; D: lanes < 16 push the carries down to their 16 lanes; W: every lane
// redoes its chunk with its carry and stores.  4 + 16 + 16 + 16 + 4 dependent steps per pass instead of len.
struct SkzgDivDesc { uint64_t src, q; uint32_t len, pad; };      // q: room for max(len - k, 0) coefficients
template <class FrP>
struct DivShortTile {
  typedef Fd<FrP> F;
  const SkzgDivDesc* desc;                // one per workgroup (device)
  const uint32_t* z; uint32_t k;          // k points (device)
  uint32_t* newton;                       // k coefficients per workgroup (device)
  static constexpr uint32_t PART = 0, CAR = SKZG_LANES, GRPV = 2 * SKZG_LANES, GRPC = 2 * SKZG_LANES + SKZG_GRP, SIDE = 2 * SKZG_LANES + 2 * SKZG_GRP;
  PC_HD uint32_t phases() const { return 5 * k + 2; }
  static PC_HD F pow2k(F v, uint32_t log2e) { for (uint32_t i = 0; i < log2e; i++) v = v.sqr(); return v; }
  static PC_HD uint32_t log2u(uint32_t v) { uint32_t l = 0; while ((1u << l) < v) l++; return l; }
  // X: the tile; S: SIDE elements; tid < SKZG_LANES always (the phases index lanes, not strides, except the copies)
  PC_HD void phase(uint32_t p, uint32_t wg, uint32_t* X, uint32_t* S, uint32_t tid) const {
    const SkzgDivDesc d = desc[wg];
    const uint32_t len = d.len, N = FrP::N;
    if (p == 0) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(d.src);
      for (uint32_t i = tid; i < len; i += SKZG_LANES) F::load(src + (size_t)i * N).store(X + (size_t)i * N);
      return;
    }
    if (p == 5 * k + 1) {
      uint32_t* q = reinterpret_cast<uint32_t*>(d.q);
      for (uint32_t i = k + tid; i < len; i += SKZG_LANES) F::load(X + (size_t)i * N).store(q + (size_t)(i - k) * N);
      if (tid < k) (tid < len ? F::load(X + (size_t)tid * N) : F::zero()).store(newton + ((size_t)wg * k + tid) * N);
      return;
    }
    const uint32_t j = (p - 1) / 5, ph = (p - 1) % 5;
    if (j >= len) return;                                             // nothing left to divide: c_j = 0
    const F zj = F::load(z + (size_t)j * N);
    const uint32_t c0 = tid * SKZG_CH, lo = c0 > j ? c0 : j, hi = c0 + SKZG_CH < len ? c0 + SKZG_CH : len;
    if (ph == 0) {
      F acc = F::zero();
      for (uint32_t i = hi; i-- > lo;) acc = F::load(X + (size_t)i * N).add(zj.mul(acc));
      acc.store(S + (size_t)(PART + tid) * N);
    } else if (ph == 1) {
      if (tid >= SKZG_GRP) return;
      const F zc = pow2k(zj, log2u(SKZG_CH));
      F acc = F::zero();
      for (uint32_t s = (tid + 1) * SKZG_GRP; s-- > tid * SKZG_GRP;) acc = F::load(S + (size_t)(PART + s) * N).add(zc.mul(acc));
      acc.store(S + (size_t)(GRPV + tid) * N);
    } else if (ph == 2) {
      if (tid != 0) return;
      const F zg = pow2k(zj, log2u(SKZG_CH * SKZG_GRP));
      F c = F::zero();
      for (uint32_t g = SKZG_GRP; g-- > 0;) { c.store(S + (size_t)(GRPC + g) * N); c = F::load(S + (size_t)(GRPV + g) * N).add(zg.mul(c)); }
    } else if (ph == 3) {
      if (tid >= SKZG_GRP) return;
      const F zc = pow2k(zj, log2u(SKZG_CH));
      F c = F::load(S + (size_t)(GRPC + tid) * N);
      for (uint32_t s = (tid + 1) * SKZG_GRP; s-- > tid * SKZG_GRP;) { c.store(S + (size_t)(CAR + s) * N); c = F::load(S + (size_t)(PART + s) * N).add(zc.mul(c)); }
    } else {
      F acc = F::load(S + (size_t)(CAR + tid) * N);
      for (uint32_t i = hi; i-- > lo;) { acc = F::load(X + (size_t)i * N).add(zj.mul(acc)); acc.store(X + (size_t)i * N); }
    }
  }
};
static_assert((SKZG_CH & (SKZG_CH - 1)) == 0, "z^CH and z^(16 CH) are made by squarings");

// r (k coefficients, HIGHEST degree first: the order of state.make_contiguous(), space.rs:133) from the Newton coefficients c_j
template <class FrP>
inline void newton_to_remainder(const uint32_t* c, const uint32_t* z, uint32_t k, uint32_t* r_high_first) {
  typedef Fd<FrP> F;
  std::vector<F> r(k, F::zero());
  for (uint32_t j = k; j-- > 0;) {                                    // r = r * (x - z_j) + c_j
    const F zj = F::load(z + (size_t)j * FrP::N);
    for (uint32_t d = k; d-- > 1;) r[d] = r[d - 1].sub(zj.mul(r[d]));
    r[0] = F::load(c + (size_t)j * FrP::N).sub(zj.mul(r[0]));
  }
  for (uint32_t d = 0; d < k; d++) r[k - 1 - d].store(r_high_first + (size_t)d * FrP::N);
}

// A tile launch: the kernels on the device, the same phases stepped lane by lane for any other backend (tests/emu)
template <class FrP, class Backend>
void launch_fold_tail(Backend&, const FoldTailTile<FrP>& t) {
  std::vector<uint32_t> A((size_t)SKZG_TILE_ELEMS * FrP::N), B((size_t)SKZG_TILE_ELEMS / 2 * FrP::N);
  for (uint32_t p = 0; p < t.phases(); p++) for (uint32_t tid = 0; tid < SKZG_LANES; tid++) t.phase(p, A.data(), B.data(), tid, SKZG_LANES);
}
template <class FrP, class Backend>
void launch_div_short(Backend&, const DivShortTile<FrP>& t, uint32_t workgroups) {
  std::vector<uint32_t> X((size_t)SKZG_TILE_ELEMS * FrP::N), S((size_t)DivShortTile<FrP>::SIDE * FrP::N);
  for (uint32_t wg = 0; wg < workgroups; wg++)
    for (uint32_t p = 0; p < t.phases(); p++) for (uint32_t tid = 0; tid < SKZG_LANES; tid++) t.phase(p, wg, X.data(), S.data(), tid);
}
#if defined(__HIPCC__)
template <class FrP>
__global__ void __launch_bounds__(SKZG_LANES) k_fold_tail(FoldTailTile<FrP> t) {
  __shared__ uint32_t A[SKZG_TILE_ELEMS * FrP::N], B[SKZG_TILE_ELEMS / 2 * FrP::N];
  PC_LATENCY_KERNEL();
  const uint32_t n = t.phases();
  for (uint32_t p = 0; p < n; p++) { t.phase(p, A, B, threadIdx.x, SKZG_LANES); __syncthreads(); }
}
template <class FrP>
__global__ void __launch_bounds__(SKZG_LANES) k_div_short(DivShortTile<FrP> t) {
  __shared__ uint32_t X[SKZG_TILE_ELEMS * FrP::N], S[DivShortTile<FrP>::SIDE * FrP::N];
  PC_LATENCY_KERNEL();
  const uint32_t n = t.phases();
  for (uint32_t p = 0; p < n; p++) { t.phase(p, blockIdx.x, X, S, threadIdx.x); __syncthreads(); }
}
template <class FrP>
void launch_fold_tail(HipBackend& be, const FoldTailTile<FrP>& t) {
  hipLaunchKernelGGL(k_fold_tail<FrP>, dim3(1), dim3(SKZG_LANES), 0, be.stream, t);
  PC_HIP_CHECK(hipGetLastError());
}
template <class FrP>
void launch_div_short(HipBackend& be, const DivShortTile<FrP>& t, uint32_t workgroups) {
  hipLaunchKernelGGL(k_div_short<FrP>, dim3(workgroups), dim3(SKZG_LANES), 0, be.stream, t);
  PC_HIP_CHECK(hipGetLastError());
}
#endif

// all `depth` levels of the tree of f (n coefficients, device) into out (device) at the element offsets offs_host[i - 1];
// returns the number of launches.  The stream is NOT drained.
template <class FrP, class Backend>
uint32_t fold_tree(Backend& be, const uint32_t* f, size_t n, const uint32_t* rho_host, uint32_t depth, uint32_t* out, const uint64_t* offs_host) {
  typedef Fd<FrP> F;
  const uint32_t* cur = f; uint32_t cur_len = (uint32_t)n, i = 1, launches = 0;
  for (; i <= depth && cur_len > SKZG_TILE_ELEMS; i++) {
    uint32_t* o = out + (size_t)offs_host[i - 1] * FrP::N;
    FoldPairBody<FrP> b{cur, cur_len, F::load(rho_host + (size_t)(i - 1) * FrP::N), o};
    cur_len = (cur_len + 1) / 2;
    be.launch(b, cur_len); launches++;
    cur = o;
  }
  if (i > depth) return launches;
  const uint32_t levels = depth - i + 1;
  const size_t rho_bytes = (size_t)levels * FrP::N * 4;
  char* args = (char*)be.workspace(rho_bytes + (size_t)levels * 8);
  be.copy_h2d(args, rho_host + (size_t)(i - 1) * FrP::N, rho_bytes);
  be.copy_h2d(args + rho_bytes, offs_host + (i - 1), (size_t)levels * 8);
  FoldTailTile<FrP> t{cur, cur_len, (const uint32_t*)args, (const uint64_t*)(args + rho_bytes), levels, out};
  launch_fold_tail<FrP>(be, t);
  return launches + 1;
}

// `count` polynomials divided by the same Z (k points on the host).  lv[i].q takes max(len - k, 0) quotient coefficients; for a
// polynomial longer than one tile the element in FRONT of q is written too (the last pass's remainder).  rem_host: count x k,
// highest degree first.  Level: {src, len, q} (SkzgDivLevel, pc_internal.hpp); scratch: skzg_div_scratch_bytes (there too).  Returns the number of launches; the stream is drained.
template <class FrP, class Backend, class Level>
uint32_t div_multi(Backend& be, const Level* lv, size_t count, const uint32_t* z_host, uint32_t k, uint32_t* rem_host, void* scratch, uint32_t fan) {
  const size_t EB = (size_t)FrP::N * 4;
  size_t max_long = 0, n_short = 0;
  for (size_t i = 0; i < count; i++) { if (lv[i].len > SKZG_TILE_ELEMS) max_long = std::max<size_t>(max_long, lv[i].len); else n_short++; }
  char* s = (char*)scratch;
  uint32_t* ping[2] = {(uint32_t*)s, (uint32_t*)(s + max_long * EB)}; s += 2 * max_long * EB;
  uint32_t* newton = (uint32_t*)s; s += count * k * EB;
  uint32_t* zdev = (uint32_t*)s; s += k * EB;
  SkzgDivDesc* ddev = (SkzgDivDesc*)s;
  uint32_t launches = 0;
  // short polynomials first in the Newton array (workgroup w of the one launch = the w-th short one); long ones behind them
  std::vector<size_t> slot(count);
  std::vector<SkzgDivDesc> descs;
  for (size_t i = 0; i < count; i++)
    if (lv[i].len <= SKZG_TILE_ELEMS) { slot[i] = descs.size(); descs.push_back(SkzgDivDesc{(uint64_t)(uintptr_t)lv[i].src, (uint64_t)(uintptr_t)lv[i].q, lv[i].len, 0u}); }
  if (n_short) {
    be.copy_h2d(zdev, z_host, k * EB);
    be.copy_h2d(ddev, descs.data(), descs.size() * sizeof(SkzgDivDesc));
    DivShortTile<FrP> t{ddev, zdev, k, newton};
    launch_div_short<FrP>(be, t, (uint32_t)n_short);
    launches++;
  }
  size_t next = n_short;
  for (size_t i = 0; i < count; i++) {
    if (lv[i].len <= SKZG_TILE_ELEMS) continue;
    slot[i] = next++;
    const uint32_t* in = lv[i].src;
    for (uint32_t j = 0; j < k; j++) {                                 // pass j: len - j coefficients in, as many out; out[0] = c_j
      const size_t m = lv[i].len - j;
      uint32_t* o = j + 1 == k ? lv[i].q - FrP::N : ping[j & 1];
      div_scan<FrP>(be, in, m, z_host + (size_t)j * FrP::N, nullptr, o, fan);
      be.copy_d2d(newton + (slot[i] * k + j) * FrP::N, o, EB);
      in = o + FrP::N;
      // the scan's own launches: an up- and a down-sweep per level of its tree (fan-in 8, then `fan`)
      size_t c = m, lvls = 0; do { c = (c + (lvls ? fan : 8) - 1) / (lvls ? fan : 8); lvls++; } while (c > 1);
      launches += 2 * (uint32_t)lvls;
    }
  }
  std::vector<uint32_t> nh(count * k * FrP::N);
  be.copy_d2h(nh.data(), newton, nh.size() * 4);
  for (size_t i = 0; i < count; i++) newton_to_remainder<FrP>(nh.data() + slot[i] * k * FrP::N, z_host, k, rem_host + i * k * FrP::N);
  return launches;
}

}  // namespace pc
