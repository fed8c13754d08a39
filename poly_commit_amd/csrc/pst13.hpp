// MarlinPST13 (poly-commit/src/marlin/marlin_pst13_pc): the device layout of a multivariate key and polynomial, and the scalar-field
// kernels on it -- the monomial evaluations of setup (mod.rs:187-207), the scatter of a sparse polynomial into a dense vector
// (from_coefficients_vec's merge of like terms), the division along one variable (divide_at_point, mod.rs:44-92) and the re-ranking
// of a key for trim (mod.rs:266-317).
//
// Layout.  n variables, total degree <= d, N(v, r) = C(v + r, v) monomials in v variables of degree <= r, M = N(n, d).  Monomials are
// ordered lexicographically by their exponent tuple (e_0 .. e_{n-1}), e_0 most significant:
//   rank(e) = sum_j [ N(v_j, r_j) - N(v_j, r_j - e_j) ],   v_j = n - j (the variables from j on),  r_j = d - (e_0 + .. + e_{j-1})
// (N(v_j, r_j) - N(v_j, r_j - e_j) tuples agree with e before j and are smaller at j: the hockey stick over N(v_j - 1, r_j - t)).
// The monomials with e_0 = .. = e_{i-1} = 0 are the prefix [0, N(n - i, d)), and on that prefix rank is the rank of (e_i .. e_{n-1})
// in the layout (n - i, d): a polynomial in X_i .. X_{n-1} occupies a prefix, and pass i of the division IS pass 0 of the layout
// (n - i, d).  The same table T[v][r] = N(v, r), v <= n, r <= d, row stride d + 1, serves every pass.
//
// Division along the leading variable of a layout (nv, d), one lane per FIBER: a fiber is a tail t = (e_1 .. e_{nv-1}) of degree
// s <= d with e_0 = k running over 0 .. d - s; fiber f is the tail of rank f in the layout (nv - 1, d) -- N(nv - 1, d) fibers.  Along
// its fiber a lane runs Horner from k = d - s down:  q[k - 1] = c[k] + z q[k]  (q[d - s] = 0), into the QUOTIENT at the slot of
// (k - 1, t), and c[0] + z q[0] into the REMAINDER at slot f -- (cur - cur|X=z) / (X - z) and cur|X=z of mod.rs:56-90, constants kept.
// Neighbouring fibers are neighbouring tails, so at equal k the lanes of a wave read and write neighbouring slots.  Every slot of
// the quotient (N(nv, d)) and of the remainder (N(nv - 1, d)) is written; nothing is assumed zeroed.
//
// The kernels keep T in LDS (at most 33 x 256 words); a body is `operator()(lane, T)`, so tests/emu steps exactly the code the
// kernels run with T in host memory.
#pragma once
#include <vector>
#include "fp32.hpp"

namespace pc {

static constexpr uint32_t PST13_MAX_VARS = 32, PST13_MAX_DEGREE = 255, PST13_LOG2_MAX_LEN = 28, PST13_LANES = 256;

// T[v][r] = C(v + r, v) for v <= n, r <= d, saturated at 2^32 - 1 (an entry a valid layout reads is at most M < 2^28)
inline std::vector<uint32_t> pst13_table(uint32_t n, uint32_t d) {
  const size_t stride = (size_t)d + 1;
  std::vector<uint32_t> T((size_t)(n + 1) * stride);
  for (uint32_t r = 0; r <= d; r++) T[r] = 1;
  for (uint32_t v = 1; v <= n; v++) {
    T[v * stride] = 1;
    for (uint32_t r = 1; r <= d; r++) {                                // N(v, r) = N(v, r - 1) + N(v - 1, r)
      const uint64_t s = (uint64_t)T[v * stride + r - 1] + T[(v - 1) * stride + r];
      T[v * stride + r] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    }
  }
  return T;
}

// the exponents of one monomial, a byte each, in registers: four named words, ALL read and masked (an indexed array of them, and
// a select between them as well, is placed in scratch memory: 36 - 40 bytes per lane in every kernel of this file)
struct Pst13Exps {
  uint64_t w0, w1, w2, w3;
  static_assert(PST13_MAX_VARS == 32, "four words of eight exponents");
  PC_HD uint32_t get(uint32_t j) const {
    const uint32_t k = j >> 3;
    const uint64_t w = (w0 & mask(k == 0)) | (w1 & mask(k == 1)) | (w2 & mask(k == 2)) | (w3 & mask(k == 3));
    return (uint32_t)(w >> ((j & 7) * 8)) & 255u;
  }
  PC_HD void set(uint32_t j, uint32_t e) {
    const uint64_t v = (uint64_t)e << ((j & 7) * 8);
    const uint32_t k = j >> 3;
    w0 |= v & mask(k == 0); w1 |= v & mask(k == 1); w2 |= v & mask(k == 2); w3 |= v & mask(k == 3);
  }
  static PC_HD uint64_t mask(bool on) { return (uint64_t)0 - (uint64_t)on; }
  PC_HD void clear() { w0 = w1 = w2 = w3 = 0; }
};

// rank of e[first .. first + nv) in the layout (nv, budget); the caller has checked that their sum is at most `budget`
PC_HD uint32_t pst13_rank(const uint32_t* T, uint32_t stride, const Pst13Exps& e, uint32_t first, uint32_t nv, uint32_t budget) {
  uint32_t rank = 0, r = budget;
  for (uint32_t j = 0; j < nv; j++) {
    const uint32_t ej = e.get(first + j);
    if (!ej) continue;
    const uint32_t* row = T + (size_t)(nv - j) * stride;
    rank += row[r] - row[r - ej];
    r -= ej;
  }
  return rank;
}
// the tuple of rank k (< N(nv, budget)) into e[first ..); returns its degree.  At most budget + nv steps.
PC_HD uint32_t pst13_unrank(const uint32_t* T, uint32_t stride, uint32_t k, uint32_t first, uint32_t nv, uint32_t budget, Pst13Exps& e) {
  uint32_t r = budget;
  for (uint32_t j = 0; j < nv; j++) {
    const uint32_t* row = T + (size_t)(nv - j) * stride;
    const uint32_t top = row[r];
    uint32_t ej = 0;
    while (ej < r && top - row[r - ej - 1] <= k) ej++;                // the largest e_j with (tuples smaller at j) <= k
    k -= top - row[r - ej];
    r -= ej;
    e.set(first + j, ej);
  }
  return budget - r;
}

// ---- bodies: operator()(lane, T) ---------------------------------------------------------------

// out[rank] = prod_j pw[j][e_j], pw: n x (d + 1) powers (pw[j][t] = beta_j^t), one lane per rank
template <class FrP>
struct Pst13MonomialBody {
  typedef Fd<FrP> F;
  const uint32_t* pw; uint32_t* out; uint32_t n, d;
  PC_HD void operator()(uint32_t lane, const uint32_t* T) const {
    Pst13Exps e; e.clear();
    pst13_unrank(T, d + 1, lane, 0, n, d, e);
    F acc = F::one();
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t ej = e.get(j);
      if (ej) acc = acc.mul(F::load(pw + ((size_t)j * (d + 1) + ej) * FrP::N));
    }
    acc.store(out + (size_t)lane * FrP::N);
  }
};

// flags of the scatter (one device word)
static constexpr uint32_t PST13_FLAG_DEGREE = 1, PST13_FLAG_REPEATED = 2;
PC_HD uint32_t pst13_load_exps(const uint8_t* bytes, uint32_t n, Pst13Exps& e) {
  uint32_t deg = 0;
  e.clear();
  for (uint32_t j = 0; j < n; j++) { e.set(j, bytes[j]); deg += bytes[j]; }
  return deg;
}
PC_HD void pst13_atomic_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  if (*p < v) *p = v;
#endif
}
PC_HD void pst13_atomic_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}
// pass 1 of the scatter, one lane per term: the slot's owner word takes the largest term index + 1 that names it
struct Pst13ClaimBody {
  const uint8_t* exps; uint32_t* owner; uint32_t* flags; uint32_t n, d;
  PC_HD void operator()(uint32_t lane, const uint32_t* T) const {
    Pst13Exps e;
    if (pst13_load_exps(exps + (size_t)lane * n, n, e) > d) { pst13_atomic_or(flags, PST13_FLAG_DEGREE); return; }
    pst13_atomic_max(owner + pst13_rank(T, d + 1, e, 0, n, d), lane + 1);
  }
};
// pass 2: the owner writes its coefficient; a term that does not own its slot is a repeated tuple (whatever the coefficients are)
template <class FrP>
struct Pst13WriteBody {
  typedef Fd<FrP> F;
  const uint8_t* exps; const uint32_t* coeffs; const uint32_t* owner; uint32_t* flags; uint32_t* out; uint32_t n, d;
  PC_HD void operator()(uint32_t lane, const uint32_t* T) const {
    Pst13Exps e;
    if (pst13_load_exps(exps + (size_t)lane * n, n, e) > d) return;
    const uint32_t slot = pst13_rank(T, d + 1, e, 0, n, d);
    if (owner[slot] != lane + 1) { pst13_atomic_or(flags, PST13_FLAG_REPEATED); return; }
    F::load(coeffs + (size_t)lane * FrP::N).store(out + (size_t)slot * FrP::N);
  }
};

// one pass of the division in the layout (nv, d): lane f = fiber f (see the head of this file).  in: N(nv, d) slots, q: as many,
// rem: N(nv - 1, d); q and rem must not overlap in.
template <class FrP>
struct Pst13DivideBody {
  typedef Fd<FrP> F;
  const uint32_t* in; uint32_t* q; uint32_t* rem; F z; uint32_t nv, d;
  PC_HD void operator()(uint32_t lane, const uint32_t* T) const {
    const uint32_t stride = d + 1, nt = nv - 1;
    Pst13Exps e; e.clear();
    const uint32_t s = pst13_unrank(T, stride, lane, 0, nt, d, e);
    const uint32_t* row = T + (size_t)nv * stride;
    F acc = F::zero();                                                  // q[d - s] = 0
    for (uint32_t k = d - s;; k--) {
      const size_t slot = (size_t)(row[d] - row[d - k]) + pst13_rank(T, stride, e, 0, nt, d - k);      // the slot of (k, tail)
      acc.store(q + slot * FrP::N);
      acc = F::load(in + slot * FrP::N).add(z.mul(acc));
      if (!k) break;
    }
    acc.store(rem + (size_t)lane * FrP::N);
  }
};

// trim: out[rank of e in (n, s)] = in[rank of e in (n, d)], s <= d, points of `aw` words; lane = a rank of the layout (n, s).
// T[v][r] does not depend on the layout: the table of (n, d) with its stride serves both
struct Pst13RerankBody {
  const uint32_t* in; uint32_t* out; uint32_t n, d, s, aw;
  PC_HD void operator()(uint32_t lane, const uint32_t* T) const {
    Pst13Exps e; e.clear();
    pst13_unrank(T, d + 1, lane, 0, n, s, e);
    const size_t src = pst13_rank(T, d + 1, e, 0, n, d);
    for (uint32_t w = 0; w < aw; w++) out[(size_t)lane * aw + w] = in[src * aw + w];
  }
};

// ---- launches: the kernel on the device, the same body stepped lane by lane for any other backend (tests/emu) ---------------
template <class Backend, class Body>
void pst13_launch(Backend&, const Body& body, size_t lanes, const uint32_t* table, uint32_t) {
  for (size_t i = 0; i < lanes; i++) body((uint32_t)i, table);
}
#if defined(__HIPCC__)
}  // namespace pc
#include "hip_backend.hpp"
namespace pc {
template <class Body>
__global__ void __launch_bounds__(PST13_LANES) k_pst13(Body body, const uint32_t* table, uint32_t table_words, uint32_t lanes) {
  extern __shared__ uint32_t pst13_T[];
  for (uint32_t i = threadIdx.x; i < table_words; i += PST13_LANES) pst13_T[i] = table[i];
  __syncthreads();
  const uint32_t lane = blockIdx.x * PST13_LANES + threadIdx.x;
  if (lane < lanes) body(lane, pst13_T);
}
template <class Body>
void pst13_launch(HipBackend& be, const Body& body, size_t lanes, const uint32_t* table_dev, uint32_t table_words) {
  if (!lanes) return;
  hipLaunchKernelGGL(k_pst13<Body>, dim3((unsigned)((lanes + PST13_LANES - 1) / PST13_LANES)), dim3(PST13_LANES), (size_t)table_words * 4, be.stream,
                     body, table_dev, table_words, (uint32_t)lanes);
  PC_HIP_CHECK(hipGetLastError());
}
#endif

// The n >= 2 passes of the division of p (N(n, d) slots, untouched) at z: quotient i (N(n - i, d) slots) at quot + offs[i] elements,
// the dividends of the passes 1 .. n-1 alternately in ping and pong (N(n - 1, d) slots each), p(z) left in slot 0 of the buffer returned.  table: T of (n, d), readable by the kernels.  The stream is NOT drained.
template <class FrP, class Backend>
const uint32_t* pst13_divide(Backend& be, const uint32_t* table, const uint32_t* T_host, uint32_t n, uint32_t d, const uint32_t* p,
                             const uint32_t* z_host, uint32_t* quot, const uint64_t* offs, uint32_t* ping, uint32_t* pong) {
  typedef Fd<FrP> F;
  const uint32_t words = (n + 1) * (d + 1);
  const uint32_t* cur = p;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t nv = n - i;
    uint32_t* rem = (i & 1) ? pong : ping;
    Pst13DivideBody<FrP> b{cur, quot + (size_t)offs[i] * FrP::N, rem, F::load(z_host + (size_t)i * FrP::N), nv, d};
    pst13_launch(be, b, T_host[(size_t)(nv - 1) * (d + 1) + d], table, words);
    cur = rem;
  }
  return cur;
}

}  // namespace pc
